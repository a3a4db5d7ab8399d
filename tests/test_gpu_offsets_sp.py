"""GPU parity of TextToIdsWithOffsets for the Unigram and BPE models: the offsets path keeps kernels of its own (Unigram: k_seg_unigram_lane +
k_uni_back, not the cut form; BPE: k_bpe_fused with its full path and the arc pool, not the wave program) and maps stream elements back to
bytes through k_prep_sp8's element -> byte map in k_compact.  Checked here at corpus scale, on long documents in batches the length sort
reorders, on byte-level BPE tokens that begin or end inside a UTF-8 character and on the device call with an output array too small: count,
ids, first byte and last byte of every checked document against the compiled reference (the oracle where oracle/_ref is not built), called
one document at a time behind a fixed byte (bfutil._T2I.with_offsets).  The same batches through TextToIdsBatch (the cut form / the wave
program) and, for the Unigram models, through BfSetVariant 6 (the forward / backward kernels the offsets path takes) give the same ids."""
import ctypes

import numpy as np
import pytest

import bfutil

bf = pytest.importorskip("blingfire_amd")
pytestmark = pytest.mark.gpu

KIND_UNIGRAM = 1
CORPORA = [("gpt2.bin", "config3", 6000), ("roberta.bin", "config3", 6000), ("xlm_roberta_base.bin", "config4", 20000),
           ("laser500k.bin", "config5", 20000), ("xlnet.bin", "config4", 20000)]
LONG_MODELS = ["gpt2.bin", "roberta.bin", "xlm_roberta_base.bin", "laser500k.bin", "xlnet.bin", "bert_base_cased_tok.bin"]


@pytest.fixture(scope="module")
def checker():
    if bfutil.have_ref():
        return bfutil.reference(), "TextToIdsWithOffsets"
    return bfutil.oracle(), "bfo_text_to_ids_with_offsets"


def _answers(ck, name, hck, text, off, sel, max_ids, unk):
    """the checker's TextToIdsWithOffsets of the documents `sel`: (counts, ids, first bytes, last bytes), the last three concatenated"""
    raw = text.tobytes()
    cnt = np.zeros(len(sel), dtype=np.int64)
    ids, st, en = [], [], []
    for k, d in enumerate(sel):
        c, i, s, e = ck.with_offsets(hck, raw[off[d]:off[d + 1]], max_ids, unk, name)
        cnt[k] = c
        ids += i
        st += s
        en += e
    return cnt, np.array(ids, dtype=np.int32), np.array(st, dtype=np.int32), np.array(en, dtype=np.int32)


def _compare(model, text, off, sel, want, got, max_ids, unk, variant):
    """got = (ids, starts, ends, id_offsets) of a batch call over the whole batch (starts / ends None: an ids call); want = _answers(...) of
    the documents sel.  Every checked document: count, ids, first bytes, last bytes"""
    cnt, wi, ws, we = want
    ids, st, en, id_off = got
    gcnt = np.diff(id_off)[sel]
    if np.array_equal(gcnt, cnt):
        first = np.repeat(id_off[sel] - np.concatenate([[0], np.cumsum(cnt)[:-1]]), cnt)
        idx = first + np.arange(int(cnt.sum()))          # the selected documents' rows of the batch output, in order
        if np.array_equal(ids[idx], wi) and (st is None or (np.array_equal(st[idx], ws) and np.array_equal(en[idx], we))):
            return
    w0 = np.concatenate([[0], np.cumsum(cnt)])
    raw = text.tobytes()
    for k, d in enumerate(sel):
        a, z = int(id_off[d]), int(id_off[d + 1])
        g = (z - a, ids[a:z].tolist(), None if st is None else st[a:z].tolist(), None if en is None else en[a:z].tolist())
        w = (int(cnt[k]), wi[w0[k]:w0[k + 1]].tolist(), None if st is None else ws[w0[k]:w0[k + 1]].tolist(),
             None if en is None else we[w0[k]:w0[k + 1]].tolist())
        if g != w:
            gt = list(zip(*[x for x in g[1:] if x is not None]))          # (id, first byte, last byte) per token
            wt = list(zip(*[x for x in w[1:] if x is not None]))
            j = next((j for j, (x, y) in enumerate(zip(gt, wt)) if x != y), min(len(gt), len(wt)))
            raise AssertionError("%s doc %d (max_ids %d unk %d variant %d, %d bytes, %r): %d tokens, the reference %d; first difference at token %d: "
                                 "gpu %s != ref %s" % (model, d, max_ids, unk, variant, int(off[d + 1] - off[d]), raw[off[d]:off[d + 1]][:60], g[0], w[0], j,
                                                       gt[j:j + 3], wt[j:j + 3]))
    raise AssertionError("%s: the id offsets differ outside the checked documents" % model)


def _check_batch(h, model, text, off, ck, name, hck, max_ids, unk, step=1):
    """TextToIdsWithOffsetsBatch (default variant) against the checker on every step-th document; TextToIdsBatch on the same batch gives the
    same ids and id offsets; for a Unigram model the ids of variant 6 equal both.  Returns (documents, tokens) compared"""
    sel = np.arange(0, len(off) - 1, step)
    want = _answers(ck, name, hck, text, off, sel, max_ids, unk)
    bf.lib().BfSetVariant(h, 3)                                             # the default of a fresh handle
    ids, st, en, id_off = bf.text_to_ids_with_offsets_batch(h, (text, off), max_ids, unk)
    _compare(model, text, off, sel, want, (ids, st, en, id_off), max_ids, unk, 3)
    ids_c, id_off_c = bf.text_to_ids_batch(h, (text, off), max_ids, unk)    # the cut form (Unigram) / the wave program (BPE) / WordPiece's ids path
    assert np.array_equal(id_off_c, id_off) and np.array_equal(ids_c, ids), (model, max_ids, "TextToIdsBatch differs from the offsets call")
    if bf.lib().BfModelKind(h) == KIND_UNIGRAM:
        bf.lib().BfSetVariant(h, 6)                                         # the forward / backward kernels from the ids API
        try:
            ids6, id_off6 = bf.text_to_ids_batch(h, (text, off), max_ids, unk)
        finally:
            bf.lib().BfSetVariant(h, 3)
        assert np.array_equal(id_off6, id_off) and np.array_equal(ids6, ids), (model, max_ids, "variant 6 differs from the default ids")
        _compare(model, text, off, sel, want, (ids6, None, None, id_off6), max_ids, unk, 6)
    return len(sel), int(want[0].sum())


@pytest.mark.parametrize("model,workload,ndocs", CORPORA)
def test_corpus_offsets(model, workload, ndocs, checker):
    """the configurations' corpora in one call per setting: the workload's max_ids / unk on every document, max_ids 16 on every seventh"""
    if not bfutil.have_model(model):
        pytest.skip("%s not present" % model)
    ck, name = checker
    wl = bfutil.WORKLOADS[workload]
    text, off = bfutil.gen_workload(workload, ndocs)
    h = bf.load_model(bfutil.model_path(model))
    hck = ck.load(bfutil.model_path(model))
    try:
        for max_ids, step in ((wl["max_ids"], 1), (16, 7)):
            nd, nt = _check_batch(h, model, text, off, ck, name, hck, max_ids, wl["unk"], step)
            print("%s %s max_ids %d: %d documents, %d tokens compared" % (model, workload, max_ids, nd, nt))
    finally:
        bf.free_model(h)
        ck.free(hck)


def _piece_edges():
    """one document whose 1:n charmap characters (and an astral one) start from three bytes before to one byte after every 512-byte piece
    boundary of k_prep_sp8, and short documents with them astride the first boundary"""
    chars = ["ª", "ﬁ", "㍿", "\U0001F600", "ﬁ㍿ª"]
    filler = b"the quick brown fox jumps over a lazy dog "
    s = bytearray()
    for j in range(1, 64):
        at = 512 * j + (j % 5) - 3
        while len(s) < at:
            s += filler[:at - len(s)]
        s += chars[j % len(chars)].encode("utf-8")
    docs = [bytes(s)]
    for k in range(505, 514):
        docs.append(b"a" * k + "ﬁ㍿ª".encode("utf-8") + " tail ﬁne".encode("utf-8") * 60)
        docs.append(b"word " * (k // 5) + b"w" * (k % 5) + "ª ﬁ ㍿".encode("utf-8") + b" end")
    return docs


def _special_docs(big_english):
    """the inputs the kernels treat apart, each a document of its own"""
    docs = []
    # BPE: single segments of far more than 4,096 arcs (k_bpe_fused's full path: k_bpe_collect_list -> k_bpe_sort -> k_bpe_apply_flat)
    docs += [b"internationalization" * 600, b"".join(w for w in big_english[:12000].split(b" ")), b"ab" * 6000]
    # Unigram: unknown runs around the 4095-position limit of the packed Viterbi record, words longer than the trie depth
    docs += [("hello " + "\U000F0000" * n + " world " + "\U000F0000" * 3 + "x").encode("utf-8") for n in (4094, 4095, 4096, 4097, 8191)]
    docs += [b"pneumonoultramicroscopicsilicovolcanoconiosis" * 40, b"x" * 3000 + b" y", ("การ" * 900).encode("utf-8")]
    # 1:n charmap characters all through a long document and at the piece edges
    docs.append(("ª ﬁ ㍿ naïve ﬁx㍿ª fiancé ﬁﬁﬁ " * 900).encode("utf-8"))
    docs += _piece_edges()
    # a BOM in front of a long document, alone, in front of one blank
    docs += [b"\xef\xbb\xbf" + big_english[:30000], b"\xef\xbb\xbf", b"\xef\xbb\xbf "]
    # invalid and truncated UTF-8 in the middle and at the end of long documents
    docs += [big_english[:20000] + b"\xff\xfe" + big_english[20000:40000], big_english[:20000] + b"\xe2\x82",
             big_english[:9000] + b"\xc3", big_english[:5000] + b"\xed\xa0\x80" + big_english[5000:9000], big_english[:4000] + b"\x80"]
    # astral characters
    docs.append(("\U0001F600 smile \U0001D4B3\U00010000 \U0010FFFF tail " * 1500).encode("utf-8"))
    # one blank, one U+2581
    docs += [b" ", "▁".encode("utf-8"), "▁".encode("utf-8") * 3000]
    return docs


@pytest.fixture(scope="module")
def long_batch():
    """the documents of test_gpu_large_docs (200 KB of English, 'a' x 100,000, 20 KB of random bytes, 45 KB of multi-byte text, 'x',
    'word ' x 20,000), the special inputs above and a few hundred short documents, interleaved: the length sort has work to do"""
    import test_gpu_large_docs
    large = test_gpu_large_docs._docs()
    longs = large + _special_docs(large[0])
    short = list(bfutil.ADVERSARIAL) + bfutil.fuzz_docs(300, seed=29)
    docs = []
    for k, d in enumerate(longs):
        docs += [d] + short[k * len(short) // len(longs):(k + 1) * len(short) // len(longs)]
    return bf.pack_docs(docs)


@pytest.mark.parametrize("model", LONG_MODELS)
def test_long_documents_offsets(model, checker, long_batch):
    if not bfutil.have_model(model):
        pytest.skip("%s not present" % model)
    ck, name = checker
    text, off = long_batch
    h = bf.load_model(bfutil.model_path(model))
    hck = ck.load(bfutil.model_path(model))
    try:
        for max_ids in (1 << 20, 1000):
            nd, nt = _check_batch(h, model, text, off, ck, name, hck, max_ids, 3)
            print("%s long batch max_ids %d: %d documents, %d tokens compared" % (model, max_ids, nd, nt))
    finally:
        bf.free_model(h)
        ck.free(hck)


def _split_character_docs():
    """documents on which byte-level BPE merges cut UTF-8 characters: emoji with skin-tone modifiers and joiners, CJK, combining marks,
    random bytes >= 0x80 and mixtures of them with ASCII"""
    rng = np.random.default_rng(31)
    pieces = ["\U0001F44D\U0001F3FD", "\U0001F468‍\U0001F469‍\U0001F467‍\U0001F466", "\U0001F3F3️‍\U0001F308",
              "\U0001F1FA\U0001F1F8", "日本語のテキスト", "中文字符", "한국어", "é", "ạ̈", "Z͑ͫ̓ͪ̂",
              "नमस्ते", "ทดสอบ", "Ünïcödé", "\U0001D4B3", " ", " ", "the", "ok,"]
    docs = []
    for k in range(1500):
        n = int(rng.integers(1, 40))
        s = "".join(pieces[int(i)] for i in rng.integers(0, len(pieces), size=n)).encode("utf-8")
        if k % 3 == 0:
            s += rng.integers(0x80, 256, size=int(rng.integers(1, 60)), dtype=np.uint8).tobytes()
        if k % 5 == 0:
            s = rng.integers(0x80, 256, size=int(rng.integers(1, 300)), dtype=np.uint8).tobytes()
        docs.append(s)
    return docs


@pytest.mark.parametrize("model", ["gpt2.bin", "roberta.bin"])
def test_byte_level_bpe_tokens_inside_characters(model, checker):
    """byte-level BPE (gpt2.bin, roberta.bin): tokens whose first byte is a UTF-8 continuation byte or whose last byte is not the end of a
    character -- their first and last bytes, like every other token's, equal the reference's; the batch must hold such tokens"""
    if not bfutil.have_model(model):
        pytest.skip("%s not present" % model)
    ck, name = checker
    text, off = bf.pack_docs(_split_character_docs())
    h = bf.load_model(bfutil.model_path(model))
    hck = ck.load(bfutil.model_path(model))
    try:
        for max_ids, unk in ((2048, 0), (5, 0)):
            nd, nt = _check_batch(h, model, text, off, ck, name, hck, max_ids, unk)
            print("%s split characters max_ids %d: %d documents, %d tokens compared" % (model, max_ids, nd, nt))
        ids, st, en, id_off = bf.text_to_ids_with_offsets_batch(h, (text, off), 2048, 0)
        doc = np.repeat(np.arange(len(off) - 1), np.diff(id_off))
        inside = (st >= 0) & ((text[np.maximum(off[doc] + st, 0)] & 0xC0) == 0x80)
        assert inside.sum() > 100, (model, int(inside.sum()), "too few tokens start inside a character")
    finally:
        bf.free_model(h)
        ck.free(hck)


@pytest.mark.parametrize("model,workload,ndocs", [("xlm_roberta_base.bin", "config4", 3000), ("gpt2.bin", "config3", 2000)])
def test_device_offsets_output_smaller_than_the_ids(model, workload, ndocs, checker):
    """TextToIdsWithOffsetsBatchDevice with cap below the need: BfLastStatus bit 0, the id offsets are complete, the documents that lie wholly
    below cap have their ids, first and last bytes, nothing is written at or beyond cap in any of the three arrays"""
    import torch
    if not bfutil.have_model(model):
        pytest.skip("%s not present" % model)
    ck, name = checker
    wl = bfutil.WORKLOADS[workload]
    max_ids, unk = wl["max_ids"], wl["unk"]
    text, off = bfutil.gen_workload(workload, ndocs)
    hck = ck.load(bfutil.model_path(model))
    try:
        cnt, wi, ws, we = _answers(ck, name, hck, text, off, np.arange(ndocs), max_ids, unk)
    finally:
        ck.free(hck)
    want_off = np.concatenate([[0], np.cumsum(cnt)])
    h = bf.load_model(bfutil.model_path(model))
    try:
        dev = torch.device("cuda", 0)
        dt, do = torch.from_numpy(text).to(dev), torch.from_numpy(off).to(dev)
        for cap in (int(want_off[-1]) - 1, int(want_off[-1]) // 2, 7):
            outs = [torch.full((cap + 64,), -7, dtype=torch.int32, device=dev) for _ in range(3)]
            ido = torch.empty(len(off), dtype=torch.int64, device=dev)
            r = bf.lib().TextToIdsWithOffsetsBatchDevice(ctypes.c_void_p(h), dt.data_ptr(), do.data_ptr(), ndocs, len(text), outs[0].data_ptr(),
                                                         outs[1].data_ptr(), outs[2].data_ptr(), cap, ido.data_ptr(), max_ids, unk,
                                                         ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
            assert r == 0
            torch.cuda.synchronize(dev)
            assert bf.lib().BfLastStatus(ctypes.c_void_p(h)) & 1, (model, cap)
            g_off = ido.cpu().numpy()
            g_ids, g_st, g_en = [t.cpu().numpy() for t in outs]
            assert np.array_equal(g_off, want_off), (model, cap)
            nfit = int(np.searchsorted(want_off, cap, side="right")) - 1          # documents [0, nfit) end at or before cap
            m = int(want_off[nfit])
            assert np.array_equal(g_ids[:m], wi[:m]) and np.array_equal(g_st[:m], ws[:m]) and np.array_equal(g_en[:m], we[:m]), (model, cap)
            assert (g_ids[cap:] == -7).all() and (g_st[cap:] == -7).all() and (g_en[cap:] == -7).all(), (model, cap)
    finally:
        bf.free_model(h)


@pytest.mark.parametrize("model", ["xlm_roberta_base.bin", "gpt2.bin"])
@pytest.mark.parametrize("tail", [0, 2])
def test_device_offsets_overflow_past_the_first_64_ids(model, tail, checker):
    """regression: k_compact set BfLastStatus bit 0 only when a document's ids ran past cap within its first 64 (one per lane), so a batch
    whose last document with ids (here followed by `tail` empty ones) crossed cap at its 65th id or later reported nothing.  Every cut of
    that document: bit 0, the complete id offsets, the first document's ids / first / last bytes, nothing at or beyond cap"""
    import torch
    if not bfutil.have_model(model):
        pytest.skip("%s not present" % model)
    ck, name = checker
    docs = [b"A short first document.", ("The offsets of a longer document, naïve ﬁne café \U0001F600. " * 30).encode("utf-8")] + [b""] * tail
    text, off = bf.pack_docs(docs)
    hck = ck.load(bfutil.model_path(model))
    try:
        cnt, wi, ws, we = _answers(ck, name, hck, text, off, np.arange(len(docs)), 4096, 0)
    finally:
        ck.free(hck)
    need, last = int(cnt.sum()), int(cnt[1])
    assert last > 130
    h = bf.load_model(bfutil.model_path(model))
    try:
        dev = torch.device("cuda", 0)
        dt, do = torch.from_numpy(text.copy()).to(dev), torch.from_numpy(off).to(dev)
        for cut in (1, 63, 64, 65, 128, last - 1):
            cap = int(cnt[0]) + cut
            outs = [torch.full((need + 64,), -7, dtype=torch.int32, device=dev) for _ in range(3)]
            ido = torch.empty(len(off), dtype=torch.int64, device=dev)
            r = bf.lib().TextToIdsWithOffsetsBatchDevice(ctypes.c_void_p(h), dt.data_ptr(), do.data_ptr(), len(docs), len(text), outs[0].data_ptr(),
                                                         outs[1].data_ptr(), outs[2].data_ptr(), cap, ido.data_ptr(), 4096, 0,
                                                         ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
            assert r == 0
            torch.cuda.synchronize(dev)
            assert bf.lib().BfLastStatus(ctypes.c_void_p(h)) & 1, (model, tail, cut)
            assert np.array_equal(ido.cpu().numpy(), np.concatenate([[0], np.cumsum(cnt)]))
            g_ids, g_st, g_en = [t.cpu().numpy() for t in outs]
            m = int(cnt[0])                                                            # the document wholly below cap
            assert np.array_equal(g_ids[:m], wi[:m]) and np.array_equal(g_st[:m], ws[:m]) and np.array_equal(g_en[:m], we[:m]), (model, cut)
            assert (g_ids[cap:] == -7).all() and (g_st[cap:] == -7).all() and (g_en[cap:] == -7).all(), (model, cut)
    finally:
        bf.free_model(h)
