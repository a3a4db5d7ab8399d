"""CPU tier under the address and undefined-behaviour sanitizers: the tokenizer lane programs (bf_lex.h, bf_seg.h, bf_wave_body.h, bf_flat_body.h,
bf_bpe_wave_body.h, bf_bpe_seg_body.h, bf_w2h.h -- the sources the kernels run) and the model loader (bf_model.cpp) as ONE stand-alone program,
tests/hosttest/bf_santest.cpp, linked from every unit of tests/hosttest, bf_model.cpp and the oracle with the flags of the four sanitized programs
of the row stage.  It is never loaded into python: the tests write case files and run it as a subprocess.

  * parity + bounds: inputs in heap blocks of exactly their size, outputs of exactly their capacity, workspaces of exactly the size the product
    reserves (tests/hosttest/ws_sizes.h, a restatement of bf_capi.cpp's arithmetic), every id, offset and count against the oracle linked into the program;
  * the loader on damaged images: truncations and 32-bit mutations of one model per family, written back through ldbedit.write_ldb so that the
    validation dump matches; every image is refused with an error text or loads, and a model that loads runs every program it is eligible for
    over a fixed 50-document catalogue within 10 x the pristine image's time + 1 s and 4 x its peak RSS.
"""
import concurrent.futures
import gzip
import json
import os
import random
import struct
import subprocess
import time

import numpy as np
import pytest

import bfutil
import flat_cases
import ldbedit
import tiny_cases
import w2h_cases

HT = os.path.join(bfutil.ROOT, "tests", "hosttest")
CSRC = os.path.join(bfutil.ROOT, "blingfire_amd", "csrc")
FLAGS = ["-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan"]
MAGIC = 0x3153434E41534642          # "BFSANCS1" (bf_santest.cpp CASE_MAGIC)
ASAN = "abort_on_error=0:detect_leaks=0:quarantine_size_mb=32"
# the loader runs: one process loads image after image, and freed blocks in quarantine count as resident -- a small quarantine, the same for the
# pristine baseline and for the damaged images, so that the RSS limit measures the images and not the quarantine
ASAN_LOADER = "abort_on_error=0:detect_leaks=0:quarantine_size_mb=4"

WP_MODELS = ["bert_base_tok.bin", "bert_base_cased_tok.bin", "bert_chinese.bin"]                                      # test_wave_emu.py, test_flat_emu.py
LEXER_MODELS = ["wbd.bin", "wbd_chuni.bin", "sbd.bin"]
UNIGRAM_MODELS = ["xlnet.bin", "xlnet_nonorm.bin", "laser50k.bin", "laser100k.bin", "xlm_roberta_base.bin", "laser500k.bin", "uri100k.bin", "uri100kint.bin"]
BPE_MODELS = ["gpt2.bin", "roberta.bin", "bpe_example.bin", "bpe_example2.bin"]                                      # test_bpe_wave_emu.py, test_bpe_seg_emu.py
DICT_MODELS = ["gpt2.bin", "roberta.bin", "xlm_roberta_base.bin", "laser500k.bin", "xlnet.bin", "bpe_example.bin", "uri100k.bin", "laser100k.bin"]      # test_dict_lookup.py


# ------------------------------------------------------------------------------------------------
# the program
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    """every unit compiled once per session, at most 16 at a time, and linked (about 75 s of compile time in all)"""
    out = tmp_path_factory.mktemp("santest")
    units = sorted(f for f in os.listdir(HT) if f.startswith("bf_") and f.endswith("test.cpp"))
    jobs = []
    for f in units:
        extra = ["-Wall", "-Wextra", "-Werror", "-DBF_SANTEST_MAIN"] if f == "bf_santest.cpp" else []
        jobs.append(["g++"] + FLAGS + extra + ["-c", os.path.join(HT, f), "-o", str(out / (f + ".o"))])
    jobs.append(["g++"] + FLAGS + ["-c", os.path.join(CSRC, "bf_model.cpp"), "-o", str(out / "bf_model.cpp.o")])
    jobs.append(["gcc"] + [x for x in FLAGS if x != "-std=c++17"] + ["-std=c99", "-c", os.path.join(bfutil.ROOT, "oracle", "bf_oracle.c"), "-o", str(out / "bf_oracle.c.o")])

    def run(cmd):
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, " ".join(cmd) + "\n" + r.stderr[-4000:]
        return cmd[-1]
    with concurrent.futures.ThreadPoolExecutor(max_workers=min(16, bfutil.host_threads())) as pool:
        objs = list(pool.map(run, jobs))
    path = str(out / "bf_santest")
    run(["g++"] + FLAGS + objs + ["-o", path])
    return path


def run_program(exe, args, timeout, asan=ASAN):
    """the program as a subprocess: a non-zero exit, a sanitizer report or a timeout fails the test, with the report's first frames"""
    env = dict(os.environ, ASAN_OPTIONS=asan, UBSAN_OPTIONS="print_stacktrace=1")
    try:
        r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, errors="replace", timeout=timeout, env=env)
    except subprocess.TimeoutExpired as e:
        pytest.fail("bf_santest %s did not finish within %d s\n%s" % (" ".join(str(a) for a in args[:2]), timeout, (e.stdout or b"")[-600:]))
    report = "\n".join(r.stderr.splitlines()[:40])
    assert r.returncode == 0 and "ERROR: AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr, \
        "exit %d\n%s\n--- stdout (end)\n%s" % (r.returncode, report, r.stdout[-800:])
    return r.stdout


def write_case(path, docs, unk=0, u_hy=0, expect=None):
    off = np.zeros(len(docs) + 1, dtype=np.int64)
    np.cumsum([len(d) for d in docs], out=off[1:])
    with open(path, "wb") as f:
        f.write(struct.pack("<8q", MAGIC, len(docs), int(off[-1]), unk, u_hy, sum(len(e) for e in expect) if expect is not None else 0, 0, 0))
        f.write(off.tobytes())
        f.write(b"".join(docs))
        if expect is not None:
            eoff = np.zeros(len(docs) + 1, dtype=np.int64)
            np.cumsum([len(e) for e in expect], out=eoff[1:])
            f.write(eoff.tobytes())
            f.write(b"".join(expect))
    return str(path)


# ------------------------------------------------------------------------------------------------
# inputs: the smallest slices of the existing catalogues that still reach each mechanism
# ------------------------------------------------------------------------------------------------
# documents whose last bytes are a truncated multi-byte character; the last one is the last bytes of the batch, where a wide load would cross the end
TRUNCATED_TAILS = [b"abc\xc3", b"word \xe2\x82", b"x" * 13 + b"\xf0\x9f\x98", b"unaffable \xe5\xa5", b"a" * 509 + b"\xe2\x82", b"the end \xf0\x9f"]


def docs_of(batch):
    text, off = batch
    raw = text.tobytes()
    return [raw[off[d]:off[d + 1]] for d in range(len(off) - 1)]


def general_docs(seed):
    """adversarial list (invalid, truncated and overlong UTF-8, BOM, NUL), fuzz documents, the truncated tails"""
    return list(bfutil.ADVERSARIAL) + bfutil.fuzz_docs(120, seed=seed) + TRUNCATED_TAILS


def tiny_docs():
    """runs of empty and one-byte documents (more than a grab of 8, more than a block of 64; all 256 byte values), words, the specials"""
    docs, _, _, _, nothers = tiny_cases.table()
    index = np.concatenate([np.zeros(tiny_cases.RUN_MIN, dtype=np.int64), np.arange(1, nothers + 1), np.zeros(9, dtype=np.int64),
                            nothers + 1 + (np.arange(150) * 7919) % (len(docs) - 1 - nothers), np.zeros(tiny_cases.RUN_MIN + 1, dtype=np.int64)])
    return docs_of(tiny_cases.pack_index(index)) + [b"\xe2\x82"]


def flat_docs():
    """streamed, handed-back, invalid and empty documents sharing blocks of 64: runs of 48 and 49 bytes at chunk boundaries, edge lengths, more words
    than a range's record list holds, many ids per document, a character outside the vocabulary as the last bytes"""
    head = flat_cases.headline(40)
    docs = flat_cases.run_docs() + flat_cases.edge_docs()[::3] + [b"", b"ab\xff cd"] + head[:20] + [flat_cases.OVERFLOW_BODIES[0][:1500], flat_cases.OVERFLOW_BODIES[3][:1500]]
    docs += flat_cases.many_docs(5) + [b""] * 3 + head[20:] + list(flat_cases.TAILS)
    return docs


def ids_case(tmp_path, model, kind):
    docs = general_docs(seed=41)
    if kind == "wp":
        docs = tiny_docs() + docs[:-1] + flat_docs() + docs[-1:]
    elif kind != "lexer":
        docs = tiny_docs()[::2] + docs
    assert docs[-1] == TRUNCATED_TAILS[-1]
    return write_case(tmp_path / "ids.case", docs, unk=100 if kind in ("wp", "lexer") else 3)


# ------------------------------------------------------------------------------------------------
# 1. parity and bounds
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,kind", [(m, "wp") for m in WP_MODELS] + [(m, "lexer") for m in LEXER_MODELS] + [(m, "unigram") for m in UNIGRAM_MODELS] + [(m, "bpe") for m in BPE_MODELS])
def test_tokenizer_programs(exe, tmp_path, model, kind):
    """per document: the lane emulation, ids and ids with offsets (Unigram: lane form, cut form at the ring sizes of test_tables_and_emu.py, sequential
    restatement); per batch: the wave program cfg 0-5 and its offsets instance, the flat program with 1, 7 and 64 ranges, the BPE wave program cfg 0
    and 1, the BPE seg program with a pool some documents overflow -- each at max_ids 0, 1, 7 and 128"""
    if not bfutil.have_model(model):
        pytest.skip("%s not present" % model)
    out = run_program(exe, ["ids", bfutil.model_path(model), ids_case(tmp_path, model, kind), 16 << 10], timeout=600)
    print(out)
    assert "ids ok:" in out
    if kind == "wp":
        assert "wave 1 flat 1" in out
    if kind == "unigram":
        assert "last key document:" in out          # the entry with the largest key: the last row of the info, score and priority tables is read
    if kind == "bpe":
        assert "bpe_wave 1 bpe_seg 1" in out
        dropped = [int(l.split()[3]) for l in out.splitlines() if l.startswith("bpe_seg small pool:")]
        assert dropped and dropped[0] > 0, "no document overflowed the small pool"


@pytest.mark.parametrize("which", ["at_the_limit", "beyond_the_limit"])
def test_flat_program_at_its_document_limit(exe, tmp_path, which):
    """a document of exactly WF_DOC_MAX bytes (the batch stays in the flat program) and one of WF_DOC_MAX + 5 among runs of tiny documents (the batch
    is not fit: every document goes to the wave program's LIST instance)"""
    model = bfutil.bert_model_name()
    if which == "at_the_limit":
        big = (b"word " * 900000)[:flat_cases.WF_DOC_MAX - 4] + b" cat"
        docs = flat_cases.headline(6) + [big] + flat_cases.headline(3) + [b"x\xe4\xb8"]
    else:
        docs = docs_of(tiny_cases.with_giant(tiny_cases.pack_index(np.concatenate([np.zeros(70, dtype=np.int64), np.arange(1, 130)]))))
    out = run_program(exe, ["flat", bfutil.model_path(model), write_case(tmp_path / "flat.case", docs, unk=100)], timeout=900)
    print(out)
    assert "flat ok:" in out


def test_flat_program_reads_nothing_behind_the_last_word(exe, tmp_path):
    """a word the table does not answer as the very last bytes of the batch (flat_cases.TAILS): k_wp_units reads it from the text, and its 16-byte
    load must stop at total_bytes"""
    for k, tail in enumerate(flat_cases.TAILS):
        docs = flat_cases.headline(12) + [b"", b"qzxjkvw zzxqj", tail]
        out = run_program(exe, ["flat", bfutil.model_path(bfutil.bert_model_name()), write_case(tmp_path / ("tail%d.case" % k), docs, unk=100)], timeout=300)
        assert "flat ok:" in out


@pytest.mark.parametrize("model", ["wbd.bin", "sbd.bin", "wbd_chuni.bin", "bert_base_cased_tok.bin"])
def test_words_and_sentences_lexers(exe, tmp_path, model):
    """the words and sentences modes, sequential program and long-document form, token for token, also with a triple buffer that fills in the middle;
    TextToWords against the oracle's"""
    docs = [d for d in general_docs(seed=43) if d] + [("д好x. Ünï çødé　text! " * 40).encode(), b"One sentence here. " * 20 + b"\n\nAnother one.", b"a b. " * 300, b"tail \xe2\x82"]
    out = run_program(exe, ["words", bfutil.model_path(model), write_case(tmp_path / "words.case", docs)], timeout=600)
    print(out)
    assert "words ok:" in out and int(out.split("words ok:")[1].split()[0]) > 200


@pytest.mark.parametrize("model", DICT_MODELS)
def test_dictionary_lookup(exe, tmp_path, model):
    if not bfutil.have_model(model):
        pytest.skip("%s not present" % model)
    import test_dict_lookup
    keys = test_dict_lookup.keys_for(model, n_random=300, seed=2)
    docs = [np.array(k, dtype=np.int64).astype(np.int32).tobytes() for k in keys]
    out = run_program(exe, ["dict", bfutil.model_path(model), write_case(tmp_path / "dict.case", docs)], timeout=300)
    print(out)
    assert int(out.split("dict ok:")[1].split()[0]) > 20 and "last key:" in out and "info id -1" not in out          # ... and the last key of the dictionary is found


def test_hyphenation_lane_program(exe, tmp_path):
    """tests/golden/w2h/syllab.bin.gz: the edge words of w2h_cases.py and a slice of the English list against the reference's stored answers"""
    en = w2h_cases.en_words()
    edge = [w for _, w in w2h_cases.edge_words()]
    for name, words, hys in (("edge", edge, w2h_cases.UHYS), ("batch_en", en, (0x2D,))):
        with gzip.open(os.path.join(bfutil.REF_ANSWERS, "word_hyphenation_%s.json.gz" % name), "rb") as f:      # the stored copy (tests/test_w2h.py holds it to the live reference)
            want = json.loads(f.read())
        for hy in hys:
            texts = [t.encode("latin-1") for t in want[str(hy)]]
            take = list(range(len(words))) if name == "edge" else list(range(0, len(words), 11))
            docs = [words[i] for i in take] + [b"abc\xe2\x82"]
            case = write_case(tmp_path / "w2h.case", docs, u_hy=hy, expect=[texts[i] for i in take] + [b""])
            out = run_program(exe, ["w2h", w2h_cases.FIXTURE, case], timeout=300)
            assert "w2h ok:" in out


# ------------------------------------------------------------------------------------------------
# 2. the loader on damaged images
# ------------------------------------------------------------------------------------------------
# family -> (image, seed, share of the mutated words that lie in the first 4 KiB of their dump, number of mutants).  The images whose load takes seconds
# under the sanitizers get fewer mutants; an [i2w] image is one array dump whose head decides everything, so its mutations lie mostly behind it
FAMILIES = {
    "lexer_bert": ("bert_base_tok.bin", 101, 0.6, 24),
    "lexer_wbd": ("wbd.bin", 102, 0.6, 60),
    "unigram": ("xlnet.bin", 103, 0.6, 60),
    "bpe": ("gpt2.bin", 104, 0.6, 40),
    "bpe_merges": ("bpe_example.bin", 105, 0.6, 40),
    "i2w": ("roberta.i2w", 106, 0.2, 200),
    "w2h": ("syllab.bin", 107, 0.6, 24),
}


def family_path(name):
    return w2h_cases.FIXTURE if name == "syllab.bin" else bfutil.model_path(name)


def truncations(raw):
    count = struct.unpack_from("<i", raw, 0)[0]
    bounds = list(struct.unpack_from("<%di" % count, raw, 4)) + [len(raw)]
    cuts = set(range(0, 17))
    for b in bounds:
        cuts.update(b + k for k in (-4, -1, 0, 1, 4))
    cuts.update(len(raw) * k // 64 for k in range(64))
    return sorted(c for c in cuts if 0 <= c < len(raw))


def mutants(path, seed, head_share, n):
    """n images: one 32-bit word inside the dumps (the configuration and the validation dump excepted) set to 0xffffffff, 0x7fffffff, 0 or a
    random value, `head_share` of them in the first 4 KiB of their dump; written back through ldbedit.write_ldb so that the validation dump matches"""
    rnd = random.Random(seed)
    dumps = ldbedit.read_ldb(path)
    conf = ldbedit.decode_conf(dumps[0])
    has_crc = ldbedit.PARAM_VERIFY_LDB_BIN in conf.get(ldbedit.FUNC_GLOBAL, [])
    targets = [i for i in range(1, len(dumps) - (1 if has_crc else 0)) if len(dumps[i]) >= 4]
    out = []
    for _ in range(n):
        ds = list(dumps)
        i = rnd.choice(targets)
        d = bytearray(ds[i])
        words = len(d) // 4
        at = rnd.randrange(min(words, 1024)) if rnd.random() < head_share else rnd.randrange(words)
        struct.pack_into("<I", d, 4 * at, rnd.choice([0xFFFFFFFF, 0x7FFFFFFF, 0, rnd.getrandbits(32)]))
        ds[i] = bytes(d)
        out.append((ds, conf))
    return out


def catalogue(tmp_path):
    docs = (list(bfutil.ADVERSARIAL[:30]) + bfutil.fuzz_docs(17, seed=5, maxwords=25) + TRUNCATED_TAILS[:3])[:50]
    assert len(docs) == 50
    words = [w for _, w in w2h_cases.edge_words()][:50]
    return write_case(tmp_path / "catalogue.case", docs, unk=3), write_case(tmp_path / "words.case", words, u_hy=0x2D)


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_loader_on_damaged_images(exe, tmp_path, family):
    """every image is refused (false and an error text) or loads; what loads runs every program its flags allow over the catalogue: no sanitizer report,
    no abort, at most 10 x the pristine image's time + 1 s per image and 4 x its peak RSS; at least 10 load and at least 10 are refused"""
    name, seed, head_share, nmut = FAMILIES[family]
    path = family_path(name)
    if not os.path.exists(path):
        pytest.skip("%s not present" % name)
    cat, words = catalogue(tmp_path)
    base = run_program(exe, ["loader", path, cat, words], timeout=600, asan=ASAN_LOADER)
    secs, rss_kb = float(base.split("baseline seconds")[1].split()[0]), int(base.split("rss_kb")[1].split()[0])
    raw = open(path, "rb").read()
    images = []
    for k, cut in enumerate(truncations(raw)):
        p = str(tmp_path / ("cut_%d.bin" % cut))
        with open(p, "wb") as f:
            f.write(raw[:cut])
        images.append(p)
    ncut = len(images)
    for k, (ds, conf) in enumerate(mutants(path, seed, head_share, nmut)):
        images.append(ldbedit.write_ldb(str(tmp_path / ("mut_%d.bin" % k)), ds, conf))
    lst = str(tmp_path / "images.txt")
    with open(lst, "w") as f:
        f.write("\n".join(images) + "\n")
    limit_mb = (4 * rss_kb + 1023) // 1024
    t0 = time.time()
    out = run_program(exe, ["loader", path, cat, words, lst], timeout=int((len(images) + 1) * (10 * secs + 1)) + 60, asan=ASAN_LOADER + ":hard_rss_limit_mb=%d" % limit_mb)
    tail = out.split("loader ok:")[1].split()
    loaded, refused = int(tail[1]), int(tail[3])
    print("%s (%s): pristine load + catalogue %.3f s, peak RSS %d KiB (limit %d MiB); %d truncations + %d mutants (seed %d, %.0f %% in the first 4 KiB): "
          "%d loaded, %d refused, slowest %s s, %.1f s wall" % (family, name, secs, rss_kb, limit_mb, ncut, nmut, seed, 100 * head_share, loaded, refused, tail[5], time.time() - t0))
    assert loaded + refused == len(images)
    assert loaded >= 10 and refused >= 10, (loaded, refused)
