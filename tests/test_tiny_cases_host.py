"""CPU: the batches of tests/tiny_cases.py -- very many tiny documents -- before the GPU tier (tests/test_gpu_tiny_documents.py) trusts them: the builders'
invariants, oracle == compiled reference on them, and the WordPiece wave program, the BPE wave program and the flat program in the wave simulator
(tests/hosttest) with ONE simulated wave opening thousands of documents, so that its table of eight open documents, the 8-bit entry number of every queued
token (bf_wave_body.h settle(): dt_head + ((entry - dt_head) & 0xFF)) and the ring base that moves with every opened document wrap dozens of times, at
1, 3 and 8 documents per grab.  BfShardRanges on batches of empty and of tiny documents is host arithmetic and runs here as well."""
import ctypes

import numpy as np
import pytest

import bfutil
import blingfire_amd as bf
import tiny_cases
from test_bpe_wave_emu import run as bpe_wave_batch
from test_flat_emu import flat_batch, flat_batch_offsets, load_hosttest
from test_wave_emu import wave_batch

N = 20000
BATCHES = ("queries", "ones")
CHECK_MODELS = ("bert_base_tok.bin", "gpt2.bin", "xlm_roberta_base.bin")
GRABS = (1, 3, 8)

_batches, _answers = {}, {}


def batch_of(name):
    if name not in _batches:
        text, off = getattr(tiny_cases, name)(N)
        index = getattr(tiny_cases, name + "_index")(N)
        for a in (text, off, index):
            a.flags.writeable = False
        _batches[name] = (text, off, index)
    return _batches[name]


def oracle_answers(model, mx, unk, offsets=False):
    """the oracle's answer for every document of tiny_cases.table(): (ids, [starts, ends,] offsets int64[ndocs + 1]) -- a document's answer depends on the
    document alone, so a batch's answer is tiny_cases.expand() of this by the batch's index"""
    key = (model, mx, unk, offsets)
    if key not in _answers:
        docs = tiny_cases.table()[0]
        ora = bfutil.oracle()
        ho = ora.load(bfutil.model_path(model))
        if offsets:
            wi, ws, we = [], [], []
            for b in docs:
                c, i_, s_, e_ = ora.with_offsets(ho, b, mx, unk, "bfo_text_to_ids_with_offsets")
                c = min(c, mx)
                wi += i_[:c]; ws += s_[:c]; we += e_[:c]
            text, off = bf.pack_docs(docs)
            _, ido = ora.batch(ho, text, off, mx, unk)
            out = (np.array(wi, dtype=np.int32), np.array(ws, dtype=np.int32), np.array(we, dtype=np.int32), ido)
            assert len(out[0]) == ido[-1]
        else:
            text, off = bf.pack_docs(docs)
            out = ora.batch(ho, text, off, mx, unk)
        ora.free(ho)
        _answers[key] = out
    return _answers[key]


def want(model, name, mx, unk, offsets=False):
    ans = oracle_answers(model, mx, unk, offsets)
    tab_off = ans[-1]
    index = batch_of(name)[2]
    start, length = tab_off[:-1], np.diff(tab_off)
    cols = [tiny_cases.expand(a, start, length, index) for a in ans[:-1]]
    return [c[0] for c in cols] + [cols[0][1]]


def first_difference(ctx, name, got_off, want_off, pairs):
    if np.array_equal(got_off, want_off) and all(np.array_equal(g, w) for _, g, w in pairs):
        return
    text, off, _ = batch_of(name)
    for d in range(len(off) - 1):
        for what, g, w in pairs:
            a, b = g[got_off[d]:got_off[d + 1]], w[want_off[d]:want_off[d + 1]]
            assert np.array_equal(a, b), (ctx, name, d, bytes(text[off[d]:off[d + 1]]), what, a.tolist(), b.tolist())
    raise AssertionError((ctx, name, "the id offsets differ behind the last document"))


@pytest.fixture(scope="module")
def ht():
    L = load_hosttest()
    L.bft_wave_ok.argtypes = [ctypes.c_void_p]
    L.bft_bpe_wave_ok.argtypes = [ctypes.c_void_p]
    L.bft_emu_wave_batch.restype = ctypes.c_long
    L.bft_emu_wave_batch.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p, ctypes.c_long, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                     ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p, ctypes.c_void_p]
    L.bft_emu_wave_batch_offsets.restype = ctypes.c_long
    L.bft_emu_wave_batch_offsets.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p, ctypes.c_long, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                             ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p]
    L.bft_emu_bpe_wave_batch.restype = ctypes.c_long
    L.bft_emu_bpe_wave_batch.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p, ctypes.c_long, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                         ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    return L


def test_builders_keep_their_invariants():
    """(the builders assert most of this themselves; here once more from the outside, at the size the simulator tier uses)"""
    text, off, index = batch_of("queries")
    lens = np.diff(off)
    assert len(lens) == N and int(lens.max()) <= 16 and len(np.unique(text)) == 256
    empty = lens == 0
    first, last, runs = tiny_cases.longest_runs(empty)
    assert first >= 70 and last >= 70 and int((runs >= 70).sum()) >= 3
    assert 0.13 <= empty.sum() / N <= 0.19
    docs = tiny_cases.table()[0]
    assert bytes(text[off[200]:off[201]]) == docs[index[200]] and all(s in docs for s in tiny_cases.SPECIALS)
    text, off, index = batch_of("ones")
    lens = np.diff(off)
    assert len(text) == N and len(lens) == N + N // 37 and set(lens.tolist()) == {0, 1} and len(np.unique(text)) == 256
    assert int((lens == 0).sum()) == N // 37 and lens[37] == 0 and lens[75] == 0
    for heavy in b"a. ":
        assert (text == heavy).sum() >= 10 * (text == ord("b")).sum()
    text, off = tiny_cases.empties(1000)
    assert len(text) == 0 and len(off) == 1001 and not off.any()
    text, off = tiny_cases.with_giant(batch_of("queries")[:2])
    lens = np.diff(off)
    assert len(lens) == N + 1 and int(lens[N // 2]) == (1 << 22) + 5 == int(lens.max()) and len(text) == off[-1]
    assert bytes(text[off[N // 2]:off[N // 2] + 12]) == b"word word wo"


@pytest.mark.parametrize("model", CHECK_MODELS)
def test_oracle_equals_the_reference_on_these_batches(model):
    """the GPU tier checks against one of the two: they have to agree on exactly these documents (ids of every document, offsets of every distinct one)"""
    if not bfutil.have_ref():
        pytest.skip("oracle/_ref is not built")
    unk = 100 if model.startswith("bert") else 3
    for name in BATCHES:
        text, off, _ = batch_of(name)
        for mx in (512, 1):
            _, ids_r, off_r = bfutil.cpu_ids_compact(bfutil.REF_LIB, bfutil.model_path(model), text, off, mx, unk)
            _, ids_o, off_o = bfutil.cpu_ids_compact(bfutil.ORACLE_LIB, bfutil.model_path(model), text, off, mx, unk)
            first_difference((model, mx, "reference (got) against oracle"), name, off_r, off_o, [("ids", ids_r, ids_o)])
            wids, woff = want(model, name, mx, unk)                       # ... and the per-table answer the simulator tests below expand
            first_difference((model, mx, "reference (got) against the expanded table"), name, off_r, woff, [("ids", ids_r, wids)])
    ref, ora = bfutil.reference(), bfutil.oracle()
    hr, ho = ref.load(bfutil.model_path(model)), ora.load(bfutil.model_path(model))
    for b in tiny_cases.table()[0]:
        for mx in (16, 1):
            assert ref.with_offsets(hr, b, mx, unk, "TextToIdsWithOffsets") == ora.with_offsets(ho, b, mx, unk, "bfo_text_to_ids_with_offsets"), (model, b, mx)
    ref.free(hr); ora.free(ho)


# what a model runs: the metric's model of each family every grab and both calls, its siblings the largest grab (a simulated run of 20,000 documents takes
# seconds, and the program is the same: the siblings differ in their tables)
@pytest.mark.parametrize("name", BATCHES)
@pytest.mark.parametrize("model", ["bert_base_tok.bin", "bert_base_cased_tok.bin", "bert_chinese.bin"])
def test_wordpiece_wave_program_one_wave_opens_every_document(ht, model, name):
    if not bfutil.have_model(model):
        pytest.skip(model)
    text, off, _ = batch_of(name)
    nd = len(off) - 1
    full = model == "bert_base_tok.bin"
    h = ht.bft_load(bfutil.model_path(model).encode())
    assert ht.bft_wave_ok(h) == 1
    try:
        for grab in (GRABS if full else GRABS[-1:]):
            for mx, unk in (((512, 100), (1, 7)) if full and grab == 3 else ((512, 100),)):
                wids, woff = want(model, name, mx, unk)
                assert int((np.diff(woff) > 0).sum()) > 10 * 256                  # one wave: its entry numbers wrap many times
                r, ids, ido, _ = wave_batch(ht, h, text, off, mx, unk, 1, grab, 3)          # 3: the shipped instance
                assert r >= 0, (model, name, grab, r)
                first_difference((model, "ids", grab, mx, unk), name, ido, woff, [("ids", ids, wids)])
            if not full:
                continue
            mx, unk = 512, 100
            wids, ws, we, woff = want(model, name, mx, unk, offsets=True)
            cap = len(text) + 16
            ids, st, en = (np.full(cap, -9, dtype=np.int32) for _ in range(3))
            ido = np.zeros(nd + 1, dtype=np.int64)
            r = ht.bft_emu_wave_batch_offsets(h, text.ctypes.data, len(text), off.ctypes.data, nd, mx, unk, 1, grab, 0, ids.ctypes.data, st.ctypes.data, en.ctypes.data,
                                              cap, ido.ctypes.data)                        # 0: the shipped OFFS instance
            assert r >= 0, (model, name, grab, r)
            first_difference((model, "offsets", grab), name, ido, woff, [("ids", ids[:r], wids), ("first bytes", st[:r], ws), ("last bytes", en[:r], we)])
    finally:
        ht.bft_free(h)


@pytest.mark.parametrize("name", BATCHES)
@pytest.mark.parametrize("model", ["gpt2.bin", "roberta.bin", "bpe_example2.bin"])
def test_bpe_wave_program_one_wave_opens_every_document(ht, model, name):
    if not bfutil.have_model(model):
        pytest.skip(model)
    text, off, _ = batch_of(name)
    # (max_ids, unk, grab, configuration): 32 = the HOME form (what ships), 0 = the in-order form
    runs = [(2048, 0, 1, 32), (2048, 0, 3, 32), (1, 1, 3, 32), (2048, 0, 8, 32), (2048, 0, 8, 0)] if model == "gpt2.bin" else [(2048, 0, 8, 32)]
    h = ht.bft_load(bfutil.model_path(model).encode())
    assert ht.bft_bpe_wave_ok(h) == 1
    try:
        for mx, unk, grab, cfg in runs:
            wids, woff = want(model, name, mx, unk)
            assert int((np.diff(woff) > 0).sum()) > 10 * 256
            r, ids, ido, fl, _ = bpe_wave_batch(ht, h, text, off, mx, unk, 1, grab, cfg)
            assert r >= 0, (model, name, grab, cfg, r)
            first_difference((model, grab, mx, unk, cfg), name, ido, woff, [("ids", ids, wids)])
    finally:
        ht.bft_free(h)


@pytest.mark.parametrize("name", BATCHES)
@pytest.mark.parametrize("model", ["bert_base_tok.bin", "bert_base_cased_tok.bin", "bert_chinese.bin"])
def test_flat_program_chunks_dense_with_documents(ht, model, name):
    """hundreds of documents per 512-byte chunk (ones(): more documents than bytes), runs of empty documents longer than k_wp_merge's block of 64"""
    if not bfutil.have_model(model):
        pytest.skip(model)
    text, off, _ = batch_of(name)
    h = ht.bft_load(bfutil.model_path(model).encode())
    assert ht.bft_flat_ok(h) == 1
    try:
        for k, (mx, unk, nw, nr) in enumerate(((512, 100, 2, 0), (1, 7, 1, 1)) if model == "bert_base_tok.bin" else ((512, 100, 3, 7),)):
            wids, ws, we, woff = want(model, name, mx, unk, offsets=True)
            if k == 0:
                r, ids, ido, _ = flat_batch(ht, h, text, off, mx, unk, nw, nr)
                assert r >= 0, (model, name, r)
                first_difference((model, "ids", mx, unk, nw, nr), name, ido, woff, [("ids", ids, wids)])
            r, ids, st, en, ido, _ = flat_batch_offsets(ht, h, text, off, mx, unk, nw, nr)
            assert r >= 0, (model, name, r)
            first_difference((model, "offsets", mx, unk, nw, nr), name, ido, woff, [("ids", ids, wids), ("first bytes", st, ws), ("last bytes", en, we)])
    finally:
        ht.bft_free(h)


@pytest.mark.parametrize("G", [2, 3, 8])
def test_shard_ranges_of_empty_and_tiny_documents(G):
    """BfShardRanges (host arithmetic: the library loads without a device) on a batch without a byte and on a batch of tiny documents"""
    for text, off in (tiny_cases.empties(1000), tiny_cases.queries(5000)):
        nd = len(off) - 1
        b = bf.shard_ranges(off, G)
        assert len(b) == G + 1 and b[0] == 0 and b[-1] == nd and np.all(np.diff(b) >= 0), (nd, G, b.tolist())
        total = int(off[-1])
        for g in range(1, G):
            if total:                                            # byte-balanced: no range is further than one document from its share
                assert abs(int(off[b[g]]) - total * g // G) <= tiny_cases.DOC_MAX, (G, g, b.tolist())
