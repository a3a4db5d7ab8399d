"""CPU: the inputs of tests/test_gpu_reserve_contract.py prove themselves (tests/reserve_cases.py) -- every batch lies within its bound, the
ones that claim to touch it touch it exactly, the long document is long in every sense a kernel switches on, and the expanding documents
really expand under the model's own charmap.  The oracle counts; no GPU."""
import ctypes

import pytest

import bfutil
import reserve_cases as rv

BOUNDS = [rv.SMALL, rv.BY_SIZE]


@pytest.mark.parametrize("D,B", BOUNDS)
def test_every_shape_is_within_its_bound_and_the_touching_ones_touch_it(D, B):
    sh = rv.shapes(D, B, pieces="xlmr")
    assert list(sh) == ["even", "one_long", "bytes", "expanding", "empty", "half"]
    for name, docs in sh.items():
        text, off = rv.pack(docs)
        assert len(docs) <= D and len(text) <= B and off[-1] == len(text), name
        if name in rv.TOUCHING:
            assert len(docs) == D and len(text) == B, (name, len(docs), len(text))
    assert len(sh["bytes"]) == min(D, B) and all(len(d) == 1 for d in sh["bytes"])
    assert sh["empty"] == []
    assert len(sh["half"]) == D // 2 and sum(len(d) for d in sh["half"]) == B // 2
    lens = [len(d) for d in sh["even"]]
    assert max(lens) - min(lens) <= 1 and min(lens) >= 1
    assert sum(1 for d in sh["one_long"] if d) == 1 and len(sh["one_long"][D // 2]) == B


def test_the_by_size_bound_passes_the_size_test_of_the_flat_program():
    D, B = rv.BY_SIZE
    assert D >= 1024 and B >= 1 << 20                     # bf_capi.cpp use_flat
    assert rv.SMALL[0] < 1024 and rv.SMALL[1] < 1 << 20  # ... and the small bound does not: there the variant chooses


@pytest.mark.parametrize("D,B", BOUNDS)
def test_the_long_document_is_long_for_every_kernel(D, B):
    doc = rv.one_long(D, B)[D // 2]
    assert len(doc) > 2048 and len(doc) > rv.long_threshold(B)
    assert all(1 <= len(w) <= 2 for w in doc.rstrip(b" ").split(b" "))      # (the cut at B bytes may leave a space at the end)
    ora = bfutil.oracle()
    h = ora.load(bfutil.model_path(bfutil.bert_model_name()))
    try:
        n, _ = ora.text_to_ids(h, doc, len(doc), 100)
    finally:
        ora.free(h)
    assert n > 1024
    for mode, model in ((1, "wbd.bin"), (2, "sbd.bin")):
        o, f = bfutil.oracle_words_fn(mode)
        hw = o.load(bfutil.model_path(model))
        try:
            r, out, _, _ = bfutil.words_call(f, (ctypes.c_void_p(hw),), doc, 2 * len(doc) + 8)
        finally:
            o.free(hw)
        assert r > 0
        if mode == 1:
            assert out[:r].count(b" ") + 1 > 1024       # words: more than 1024 of them, so k_w2t_copy_long assembles the document


@pytest.mark.parametrize("D,B", BOUNDS)
def test_the_expanding_documents_expand_under_the_models_charmap(D, B):
    ora = bfutil.oracle()
    get = ora.lib.bfo_charmap_get
    get.restype = ctypes.c_int
    get.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int]
    h = ora.load(bfutil.model_path("xlm_roberta_base.bin"))
    buf = (ctypes.c_int * 32)()
    width = {}
    try:
        chars = rv.expanding_chars("xlmr")
        assert len(chars) >= 20
        for c in chars:
            n = get(ctypes.c_void_p(h), 1, ord(c.decode("utf-8")), buf, 32)
            width[c] = n if n >= 0 else 1
            assert width[c] > len(c), (c, n)              # every chosen character: more stream elements than bytes
        docs = rv.expanding(D, B, "xlmr")
        elements = 0
        for d in docs:
            elements += sum(width.get(ch.encode("utf-8"), 1) for ch in d.decode("utf-8"))
        assert elements > B == sum(len(d) for d in docs), (elements, B)
    finally:
        ora.free(h)


def test_the_stored_hyphenation_answers_are_those_of_the_shapes():
    """the fixture of the hyphenation case belongs to the words reserve_cases builds today: one answer per word, equal to the live reference where
    oracle/_ref is built; an answer holds its word's characters (the first 300: what lies behind them is never looked at) and hyphens between them"""
    want = rv.hyphenation_expected()
    words = rv.hyphenation_words()
    assert list(want) == list(words)
    for name, docs in words.items():
        assert len(want[name]) == len(docs), name
        for w, t in zip(docs, want[name]):
            assert t == "" or min(len(w), 300) <= len(t) <= 2 * len(w), (name, w[:40], len(t))
    assert any("-" in t for t in want["even"])


def test_the_stream_stage_has_more_rows_than_sequences_on_the_long_shape():
    """IdsToStreamRowsBatchDevice claims that no workspace of its is sized by the row count: the shape that tries it has several times as many rows as
    sequences, all of them inside the reserved number of sequences; the count is the sequential restatement's"""
    import packed_cases
    import stream_cases
    D = rv.SMALL[0]
    lens = rv.seq_shapes(D, long_len=300)["one_long"]
    assert len(lens) == D
    ids, off = packed_cases.ragged(lens)
    counts = []
    for L in rv.STREAM_ROW_LENS:
        R = stream_cases.restate(ids, off, L, stream_cases.BOS, stream_cases.EOS)[8]
        assert R == rv.stream_row_count(lens, L) == stream_cases.restate_np(ids, off, L, stream_cases.BOS, stream_cases.EOS)[8]
        counts.append(R)
    assert max(counts) > 3 * D, counts
    for name, lens in rv.seq_shapes(D, long_len=300).items():
        assert len(lens) <= D, name
