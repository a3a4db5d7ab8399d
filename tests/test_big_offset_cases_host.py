"""CPU tier of tests/test_gpu_beyond_2gib.py: tests/big_offset_cases.py is held to the reference and to its own claims.

  1  the reference refuses a document of more than 10^9 bytes in every entry point the GPU tests call, with the answer the tests expect of the
     filler documents (nothing), and without reading the text: the call gets 2^30 bytes of an anonymous mapping that no one has touched, returns
     at once and leaves the process's resident memory where it was.  (blingfiretokdll.cpp:198, 449, 835, 1121, 1362 compare the byte count with
     FALimits::MaxArrSize before the first allocation; read there, checked here.)
  2  the real documents are what the module says, and the two checkers agree on them
  3  the fillers put every real document's byte offset, staging slot and workspace cell behind 2^31
  4  the arithmetic of batch C
  5  the memory helper: the model facts it uses are the loader's, its sums are those of bf_capi.cpp on hand-computed cases"""
import ctypes
import mmap
import time

import numpy as np
import pytest

import bfutil
import big_offset_cases as bo

VP, CI = ctypes.c_void_p, ctypes.c_int
MODELS = [m for m in bo.FACTS if bfutil.have_model(bo.model_file(m))]


def _rss():
    with open("/proc/self/statm") as f:
        return int(f.read().split()[1]) * mmap.PAGESIZE


class Untouched:
    """2^30 bytes nobody has written: pages come into being only when something reads or writes them"""

    def __enter__(self):
        self.mm = mmap.mmap(-1, bo.GIB, flags=mmap.MAP_PRIVATE | mmap.MAP_ANONYMOUS)
        self.view = ctypes.c_char.from_buffer(self.mm)
        self.addr = ctypes.addressof(self.view)
        self.before = _rss()
        return self

    def __exit__(self, *a):
        grown = _rss() - self.before
        del self.view
        self.mm.close()
        assert grown < (64 << 20), "the call read the text: resident memory grew by %d bytes" % grown


def _outs(n=8):
    return [(ctypes.c_int32 * n)(*([-7] * n)) for _ in range(3)]


def _untouched(*arrays):
    return all(list(a) == [-7] * len(a) for a in arrays)


# ---- 1. the 10^9 rule
def _over_limit_answers(lib, names, load, free, with_model_first):
    """{entry point: [return value, outputs untouched]} for a document of 2^30 bytes"""
    out = {}
    with Untouched() as u:
        for model in MODELS:
            h = load(bfutil.model_path(bo.model_file(model)))
            try:
                ids, st, en = _outs()
                f = getattr(lib, names["ids"]); f.restype = CI; f.argtypes = [VP, VP, CI, VP, CI, CI]
                out["TextToIds " + model] = [f(VP(h), u.addr, bo.GIB, ids, 8, 0), _untouched(ids)]
                f = getattr(lib, names["offsets"]); f.restype = CI; f.argtypes = [VP, VP, CI, VP, VP, VP, CI, CI]
                out["TextToIdsWithOffsets " + model] = [f(VP(h), u.addr, bo.GIB, ids, st, en, 8, 0), _untouched(ids, st, en)]
            finally:
                free(h)
        for what, default in (("words", "wbd.bin"), ("sentences", "sbd.bin")):
            buf = ctypes.create_string_buffer(b"\x7f" * 16, 16)
            ids, st, en = _outs()
            f = getattr(lib, names[what]); f.restype = CI
            if with_model_first:
                h = load(bfutil.model_path(default))
                f.argtypes = [VP, VP, CI, VP, VP, VP, CI]
                r = f(VP(h), u.addr, bo.GIB, buf, st, en, 16)
                free(h)
            else:
                f.argtypes = [VP, CI, VP, VP, VP, CI, VP]
                r = f(u.addr, bo.GIB, buf, st, en, 16, None)     # NULL: the built-in model
            out["TextTo%s built-in" % what.capitalize()] = [r, buf.raw == b"\x7f" * 16 and _untouched(st, en)]
        if "hyphenation" in names:
            import w2h_cases as wc
            h = load(wc.FIXTURE)
            buf = ctypes.create_string_buffer(b"\x7f" * 16, 16)
            f = getattr(lib, names["hyphenation"]); f.restype = CI; f.argtypes = [VP, CI, VP, CI, VP, CI]
            out["WordHyphenation"] = [f(u.addr, bo.GIB, buf, 16, VP(h), 0x2D), buf.raw == b"\x7f" * 16]
            free(h)
    return out


def _expected_over_limit():
    e = {}
    for model in MODELS:
        e["TextToIds " + model] = [0, True]
        e["TextToIdsWithOffsets " + model] = [0, True]
    e["TextToWords built-in"] = [-1, True]
    e["TextToSentences built-in"] = [-1, True]
    return e


def test_1_the_reference_refuses_a_document_over_its_limit_before_reading_it():
    """what the GPU tests expect of a filler A document -- no ids, no words, no sentences, no hyphenated word -- is the compiled reference's answer"""
    assert bo.FILLER_A == (bo.GIB, bo.GIB) and bo.GIB > bo.LIMIT

    def compute():
        ref = bfutil.reference()
        names = dict(ids="TextToIds", offsets="TextToIdsWithOffsets", words="TextToWordsWithOffsetsWithModel", sentences="TextToSentencesWithOffsetsWithModel",
                     hyphenation="WordHyphenationWithModel")
        return _over_limit_answers(ref.lib, names, ref.load, ref.free, False)
    got = bfutil.reference_answers("big_offset_over_limit", compute)
    want = _expected_over_limit()
    want["WordHyphenation"] = [-1, True]
    want = {k: v for k, v in want.items()}
    assert {k: got[k] for k in want} == want


def test_1_the_oracle_restates_the_rule():
    """the checker of a machine without oracle/_ref answers the same, as early"""
    ora = bfutil.oracle()
    names = dict(ids="bfo_text_to_ids", offsets="bfo_text_to_ids_with_offsets", words="bfo_text_to_words_with_offsets", sentences="bfo_text_to_sentences_with_offsets")
    assert _over_limit_answers(ora.lib, names, ora.load, ora.free, True) == _expected_over_limit()


# ---- 2. the real documents
def test_2_real_documents_are_what_the_module_says():
    docs = bo.real_docs()
    assert docs[:len(bfutil.ADVERSARIAL)] == tuple(bfutil.ADVERSARIAL) and len(docs) == len(bfutil.ADVERSARIAL) + 300 + 6
    sizes = sorted(len(d) for d in docs)
    assert sizes[0] == 0 and 1 in sizes and sizes[-1] > 4096 and sum(1 for s in sizes if 2048 < s <= 4096) >= 1 and sizes[-1] <= bo.WF_DOC_MAX
    assert docs[-1] == bo.TRUNCATED_TAIL and docs[-1].endswith(b"\xe2\x82") and docs[-2] == b""
    words, woff = bo.expected_text(1)
    k = max(range(len(docs)), key=lambda d: len(docs[d]))
    assert bytes(words[woff[k]:woff[k + 1]]).count(b" ") + 1 > 1024          # more tokens than w2t_list_long's threshold
    for model in MODELS:
        ids, id_off = bo.expected_ids(model)
        assert int(np.diff(id_off).max()) < bo.MAX_IDS and id_off[-1] == len(ids) > 5000      # nothing is cut by max_ids
        if bo.family(model) == "wp":
            assert id_off[-1] - id_off[-2] == 0                  # invalid UTF-8: a WordPiece document answers nothing (tokdll:1151-1153)


@pytest.mark.skipif(not bfutil.have_ref(), reason="compares the two checkers: needs oracle/_ref")
@pytest.mark.parametrize("model", MODELS)
def test_2_oracle_and_reference_agree_on_the_real_documents(model):
    """the GPU tier takes the oracle where oracle/_ref is absent: on these documents it is the reference"""
    ora = bfutil.oracle()
    h = ora.load(bfutil.model_path(bo.model_file(model)))
    try:
        text, off = bo.pack(bo.real_docs())
        ids, id_off = ora.batch(h, text, off, bo.MAX_IDS, bo.UNK[bo.family(model)])
        wids, woff = bo.expected_ids(model)
        assert np.array_equal(id_off, woff) and np.array_equal(ids, wids)
        oi, os_, oe, ooff = bo.expected_offsets(model)
        k = 0
        for d, b in enumerate(bo.real_docs()):
            c, i_, s_, e_ = ora.with_offsets(h, b, min(bo.MAX_IDS, len(b) + 1), bo.UNK[bo.family(model)], "bfo_text_to_ids_with_offsets")
            a, z = int(ooff[d]), int(ooff[d + 1])
            assert (list(i_), list(s_), list(e_)) == (oi[a:z].tolist(), os_[a:z].tolist(), oe[a:z].tolist()), (model, d, b[:60])
            k += c
        assert k == ooff[-1]
    finally:
        ora.free(h)


@pytest.mark.skipif(not bfutil.have_ref(), reason="compares the two checkers: needs oracle/_ref")
@pytest.mark.parametrize("mode", [1, 2])
def test_2_oracle_and_reference_agree_on_words_and_sentences(mode):
    import secondary_cases as sc
    ora = sc.Checker(use_ref=False)
    fn = ora.words if mode == 1 else ora.sentences
    flat, off = bo.pack([fn(b) for b in bo.real_docs()])
    wflat, woff = bo.expected_text(mode)
    assert np.array_equal(off, woff) and np.array_equal(flat, wflat)


def test_2_filler_b_documents_answer_as_the_module_says():
    """one document of 4 MiB of spaces: no ids with a WordPiece model, the dummy prefix alone with a Unigram model; the time is printed (the module's
    docstring records it: filler B is for programs whose reference answers such a document in about a second)"""
    ck = bo.checker()
    doc = b" " * bo.WF_DOC_MAX
    for model, want in (("bert", 0), ("xlm_roberta_base.bin", 1)):
        h = ck.load(bfutil.model_path(bo.model_file(model)))
        try:
            t = time.time()
            c, buf = ck.text_to_ids(h, doc, 16, bo.UNK[bo.family(model)])
            print("%s: %d ids of 4 MiB of spaces in %.3f s" % (model, c, time.time() - t))
            assert c == want == bo.FILLER_B_IDS[bo.family(model)]
            if want:
                one, _ = ck.text_to_ids(h, b" ", 16, bo.UNK[bo.family(model)])
                assert one == 1 and buf[0] == ck.text_to_ids(h, b" ", 16, bo.UNK[bo.family(model)])[1][0] == bo.filler_b_id(model)
        finally:
            ck.free(h)


# ---- 3. where the fillers put the real documents
@pytest.mark.parametrize("filler", ["A", "B"])
def test_3_every_real_document_lies_behind_two_gib(filler):
    off, nfill = bo.batch_offsets(filler)
    assert off.dtype == np.int64 and off[nfill] == bo.TWO31 and (off[nfill:] >= bo.TWO31).all() and (np.diff(off) >= 0).all()
    assert len(off) - 1 == nfill + len(bo.real_docs()) and off[-1] == bo.TWO31 + sum(len(d) for d in bo.real_docs())
    lens = np.diff(off[:nfill + 1])
    if filler == "A":
        assert nfill == 2 and (lens > bo.LIMIT).all() and (lens < bo.TWO31).all()
    else:
        assert nfill == 512 and (lens == bo.WF_DOC_MAX).all() and int(np.diff(off).max()) == bo.WF_DOC_MAX      # the flat program takes the batch
    d = np.arange(nfill, len(off) - 1, dtype=np.int64)
    assert ((((off[d] + 7) & ~7) + 8 * d) >= bo.TWO31).all()     # bf_wave.h wv_ids_slot
    for mul in (1, 2):
        assert (mul * (off[d] + d) >= mul * bo.TWO31).all()      # bf_kernels_sp.hip sp_slot
    assert int(2 * (off[-1] + len(off) - 1) + 64) > 1 << 32      # reserve_sp_workspaces' `cap` with a charmap: more than 2^32 elements
    woff = bo.with_filler(np.array([0, 3, 3, 10], dtype=np.int64), nfill, 1 if filler == "B" else 0)
    assert len(woff) == nfill + 4 and woff[nfill] == (nfill if filler == "B" else 0) and woff[-1] == woff[nfill] + 10


# ---- 4. batch C
def test_4_batch_c_arithmetic():
    assert len(bo.C_DOC) == 512 and bo.C_DOC.split() == [bytes([97 + i % 26]) for i in range(255)]
    ids, id_off = None, None
    ck = bo.checker()
    h = ck.load(bfutil.model_path(bo.model_file("bert")))
    try:
        k, buf = ck.text_to_ids(h, bo.C_DOC, 512, 100)
    finally:
        ck.free(h)
    assert k == bo.C_WORDS == 255 and 100 not in buf[:k]         # every letter is in the vocabulary
    c = bo.batch_c(k)
    n = c["ndocs"]
    assert c["total_ids"] == n * k > bo.C_MIN_IDS >= (n - 1) * k and n < (1 << 31)
    assert c["total_bytes"] == n * 512 > (1 << 32)
    s = c["straddler"]
    assert s * k < bo.TWO31 < (s + 1) * k                        # ids on both sides of output position 2^31
    id_off = np.arange(n + 1, dtype=np.int64) * k                # the expected id offsets: int64, the last ones beyond 2^31
    assert id_off.dtype == np.int64 and id_off[-1] == c["total_ids"] and id_off[s] < bo.TWO31 < id_off[s + 1]
    assert (id_off[-1].astype(np.int32) != id_off[-1])           # (and not representable in 32 bits)
    cap = bo.TWO31 + 5
    whole, below = bo.batch_c_capped(k, cap)
    assert whole * k <= cap < (whole + 1) * k and below == cap and whole == s       # the straddler is the document the cap cuts
    assert bo.batch_c(256)["straddler"] is None                  # (a document of 256 ids would begin exactly at 2^31: 255 is on purpose)


# ---- 5. the memory helper
def test_5_model_facts_are_the_loaders():
    from test_flat_emu import load_hosttest
    ht = load_hosttest()
    ht.bft_reserve_facts.argtypes = [VP, VP]
    ht.bft_kind.argtypes = [VP]
    kinds = {"wp": (0,), "unigram": (1,), "bpe": (2, 3, 4)}      # bf_model.h ModelKind
    for model in MODELS:
        h = ht.bft_load(bfutil.model_path(bo.model_file(model)).encode())
        try:
            out = (ctypes.c_int * 4)()
            ht.bft_reserve_facts(VP(h), out)
            fam, mul, rec, bwave = bo.FACTS[model]
            assert ht.bft_kind(VP(h)) in kinds[fam], (model, ht.bft_kind(VP(h)))
            if fam == "wp":
                assert out[3] == 1, model                        # the flat program applies
            else:
                assert out[0] == mul and out[2] == bwave, (model, list(out))
            if fam == "unigram":
                assert out[1] == rec, (model, list(out))
        finally:
            ht.bft_free(h)


def test_5_memory_helper_on_hand_computed_cases():
    B, D = bo.TWO31 + 100000, 400
    grow = lambda n: n + n // 8 + 256
    # the wave program, ids only, of a WordPiece handle: BfReserve also sizes the words modes (14 bytes per byte of text) and the words outputs (12)
    r = bo.reserved_bytes("bert", D, B, False, 5)
    big = grow((B + 8 * D + 64) * 4) + grow((B + 64) * 2) + grow((B + 64) * 4) + grow((B + 8 * D + 64) * 8) + 3 * grow((B + 1) * 4)
    assert big < r < big + (2 << 30)
    # the flat program with offsets adds entries, homes and their spans: 4 + 4 + 4 + 8 bytes per byte
    rf = bo.reserved_bytes("bert", D, B, True, 4)
    assert rf - r > grow((B + 64) * 4) * 3 + grow((B + 64) * 8) - (1 << 20)
    # a Unigram model with a charmap: two stream elements per byte -- 2 + 4 + 4 bytes each, the offsets API 4 + 8 more
    u = bo.reserved_bytes("xlm_roberta_base.bin", D, B, False)
    cap = 2 * (B + D) + 64
    assert cap > 1 << 32
    assert grow(cap * 2 + 512) + grow(cap * 4) * 2 < u < grow(cap * 2 + 512) + grow(cap * 4) * 2 + (2 << 30)
    assert bo.reserved_bytes("xlm_roberta_base.bin", D, B, True) - u > grow(cap * 4) + grow(cap * 8) - (1 << 20)
    # the lane-per-document BPE kernels: what the module leaves out, and why
    lane = bo.reserved_bytes("gpt2.bin", D, B, True)
    assert lane > 250 * 10 ** 9 > bo.reserved_bytes("gpt2.bin", D, B, False) * 3
    assert not bo.enough_memory(bo.device_bytes("gpt2.bin", D, B, True, out_cells=10000, out_arrays=3), 288 * 10 ** 9)
    # every case of the GPU matrix fits an idle 288 GB device with the 10 % to spare
    for model, want_off, variant in (("bert", True, 4), ("bert", True, 2), ("xlm_roberta_base.bin", True, 3), ("xlnet.bin", False, 3), ("gpt2.bin", False, 3)):
        assert bo.enough_memory(bo.device_bytes(model, D, B, want_off, variant, out_cells=20000, out_arrays=3), 280 * 10 ** 9), (model, want_off, variant)
    c = bo.batch_c(255)
    need = bo.device_bytes("bert", c["ndocs"], c["total_bytes"], False, 4, out_cells=c["total_ids"]) + c["total_ids"]       # (+ the comparison's byte per id)
    assert bo.enough_memory(need, 280 * 10 ** 9), need
    assert bo.enough_memory(100, 110) and not bo.enough_memory(100, 109)
