"""Word hyphenation ([w2h] models: tests/golden/w2h/syllab.bin.gz, unpacked by w2h_cases): the loader, the host build of the lane programs (bf_w2h.h through
tests/hosttest/bf_w2htest.cpp, CPU tier) and the product library's WordHyphenationWithModel / WordHyphenationBatch / WordHyphenationBatchDevice
(GPU tier) against the unmodified reference's WordHyphenationWithModel (tokdll:818-911 over FAHyphInterpreter_core_t.h:136-267).

Every expectation is the reference's own answer, asked per word through oracle/_ref where that is built and taken from its stored copy
(tests/golden/ref_answers/word_hyphenation_*.json.gz, bfutil.reference_answers) elsewhere.  Comparisons are exact -- the return value and
every byte -- and no word is left out of one."""
import ctypes

import numpy as np
import pytest

import bfutil
import secondary_cases as sc
import w2h_cases as wc

VP, CI = ctypes.c_void_p, ctypes.c_int
E_ARG, E_UNSUPPORTED = -1, -5


# ------------------------------------------------------------------------------------------------
# the host build (CPU tier)
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def H():
    L = ctypes.CDLL(bfutil.HOSTTEST_LIB)
    L.bft_load.restype = VP
    L.bft_load.argtypes = [ctypes.c_char_p]
    L.bft_error.restype = ctypes.c_char_p
    L.bft_error.argtypes = L.bft_free.argtypes = L.bft_kind.argtypes = L.bft_w2h_ready.argtypes = [VP]
    L.bft_w2h_facts.argtypes = [VP, VP]
    L.bft_w2h_one.argtypes = [VP, ctypes.c_char_p, CI, VP, CI, CI]
    L.bft_w2h_batch.restype = ctypes.c_longlong
    L.bft_w2h_batch.argtypes = [VP, VP, VP, ctypes.c_longlong, CI, VP, ctypes.c_longlong, VP]
    return L


def host_batch(H, h, words, hy, cap=None):
    flat, off = sc.pack(words)
    out_off = np.full(len(words) + 1, -1, dtype=np.int64)
    n = H.bft_w2h_batch(VP(h), flat.ctypes.data, off.ctypes.data, len(words), hy, None, 0, out_off.ctypes.data)
    if n < 0:
        return n, None, None
    out = np.full(n + 64, 0xA5, dtype=np.uint8)
    assert H.bft_w2h_batch(VP(h), flat.ctypes.data, off.ctypes.data, len(words), hy, out.ctypes.data, n if cap is None else cap, out_off.ctypes.data) == n
    return n, out, out_off


def same_texts(out, out_off, want, words, what):
    w_flat, w_off = wc.pack_texts(want)
    assert np.array_equal(out_off, w_off), sc.first_difference(out_off, w_off, sc.pack(words), what)
    got = out[:w_off[-1]]
    if not np.array_equal(got, w_flat):
        bad = int(np.nonzero(got != w_flat)[0][0])
        d = int(np.searchsorted(w_off, bad, side="right") - 1)
        raise AssertionError("%s: word %d %r: got %r, the reference %r" % (what, d, words[d][:60], got[w_off[d]:w_off[d + 1]].tobytes(), want[d]))


def facts(H, h):
    a = (CI * 10)()
    H.bft_w2h_facts(VP(h), a)
    return dict(zip(("has", "ready", "ignore_case", "min_len", "min_len2", "left", "right", "classes", "entries", "pattern_bytes"), a))


def test_1_loader_accepts_the_fixture_and_its_variants(H, tmp_path):
    h = H.bft_load(wc.FIXTURE.encode())
    assert H.bft_error(VP(h)) == b"" and H.bft_kind(VP(h)) == 6
    f = facts(H, h)
    assert (f["has"], f["ready"], f["ignore_case"], f["min_len"], f["min_len2"], f["left"], f["right"]) == (1, 1, 0, 2, 0, 94, 94)
    assert f["classes"] > 100 and f["entries"] > 100000 and f["pattern_bytes"] > 1000
    H.bft_free(VP(h))
    want = {"ignore_case": ("ignore_case", 1), "min_len2_1": ("min_len2", 1), "min_len2_2": ("min_len2", 2), "min_len2_5": ("min_len2", 5),
            "min_len_8": ("min_len", 8), "min_len_20": ("min_len", 20)}
    for name in wc.VARIANTS:
        h = H.bft_load(wc.make_variant(name, tmp_path).encode())
        assert H.bft_error(VP(h)) == b"" and H.bft_kind(VP(h)) == 6, name
        assert facts(H, h)[want[name][0]] == want[name][1], name
        H.bft_free(VP(h))


def test_1_loader_refuses_what_the_reference_refuses(H, tmp_path):
    for name, word in (("unknown_parameter", b"unknown parameter 38"), ("zero_anchor", b"left-anchor"), ("min_len_0", b"min-len")):
        h = H.bft_load(wc.make_variant(name, tmp_path).encode())
        assert word in H.bft_error(VP(h)), (name, H.bft_error(VP(h)))
        H.bft_free(VP(h))


def test_1_loader_refuses_a_pattern_value_the_parallel_overlay_cannot_hold(H, tmp_path):
    """HYPH_UNKNOWN / HYPH_CONFLICT (or anything else outside 0 .. 7) as a pattern value makes the reference's overlay depend on its order
    (the [w2h] section): such a model is refused at load with a message, not hyphenated differently"""
    for value in (-1, -2, 8):
        h = H.bft_load(wc.make_bad_pattern_value(tmp_path, value).encode())
        err = H.bft_error(VP(h))
        assert b"pattern 0 holds the value %d" % value in err and b"order" in err, err
        H.bft_free(VP(h))


def test_2_host_single_call_equals_the_reference(H):
    rows = wc.table_rows()
    want = wc.ref_singles("table", wc.FIXTURE, rows)
    h = H.bft_load(wc.FIXTURE.encode())
    for (w, hy, cap), exp in zip(rows, want):
        assert wc.single(H.bft_w2h_one, h, w, hy, cap, first=True) == exp, (w[:40], hex(hy), cap)
    H.bft_free(VP(h))


def capacity_rows():
    rows = []
    for w in wc.capacity_words():
        for hy in (0x2D, 0x2581):
            need = len(w) + 16 * 4
            rows += [(w, hy, cap) for cap in range(0, need)]
    return rows


def _full_need(want_rows, rows):
    """capacities run from 0 to beyond needed + 1 for every word (the builder over-counts; this pins that it does)"""
    for w in wc.capacity_words():
        rets = [exp[0] for (ww, hy, cap), exp in zip(rows, want_rows) if ww == w and hy == 0x2D]
        assert rets[-1] == rets[-2] and rets[-1] <= len(rets) - 2 and rets[0] == rets[-1] - 1


def test_2_host_every_capacity_equals_the_reference(H):
    rows = capacity_rows()
    want = wc.ref_singles("capacities", wc.FIXTURE, rows)
    _full_need(want, rows)
    h = H.bft_load(wc.FIXTURE.encode())
    for (w, hy, cap), exp in zip(rows, want):
        assert wc.single(H.bft_w2h_one, h, w, hy, cap, first=True) == exp, (w, hex(hy), cap)
    H.bft_free(VP(h))


@pytest.mark.parametrize("name", ["en", "en_upper", "en_capitalised", "corpus"])
def test_2_host_batch_equals_the_reference(H, name):
    words = wc.batch_lists()[name]
    want = wc.ref_texts("batch_" + name, wc.FIXTURE, words)["45"]
    if name == "en":
        assert len(words) == 21719 and "" not in want and sum(len(t) > len(w) for t, w in zip(want, words)) == 16492
    h = H.bft_load(wc.FIXTURE.encode())
    n, out, off = host_batch(H, h, words, 0x2D)
    same_texts(out, off, want, words, "host build, " + name)
    H.bft_free(VP(h))


def test_2_host_edge_words_and_hyphens_equal_the_reference(H):
    words = [w for _, w in wc.edge_words()]
    want = wc.ref_texts("edge", wc.FIXTURE, words, wc.UHYS)
    h = H.bft_load(wc.FIXTURE.encode())
    for hy in wc.UHYS:
        n, out, off = host_batch(H, h, words, hy)
        same_texts(out, off, want[str(hy)], words, "host build, edge words, uHy 0x%x" % hy)
        # the capacity guard of the copy: nothing at or past a capacity inside the output
        n2, out2, off2 = host_batch(H, h, words, hy, cap=n // 2)
        assert np.array_equal(out2[:n // 2], out[:n // 2]) and (out2[n // 2:] == 0xA5).all()
    for hy in wc.BAD_UHYS:
        assert host_batch(H, h, words, hy)[0] == -1
    H.bft_free(VP(h))


def variant_answers(name, path):
    return wc.ref_texts("variant_" + name, path, wc.variant_words())["45"]


@pytest.mark.parametrize("name", list(wc.VARIANTS))
def test_2_host_model_variants_equal_the_reference(H, name, tmp_path):
    words = wc.variant_words()
    want = variant_answers(name, wc.make_variant(name, tmp_path))
    base = wc.ref_texts("variant_base", wc.FIXTURE, words)["45"]
    assert want != base, "the variant %s exercises nothing on these words" % name
    told = {"ignore_case": ["hel-lo", "syl-la-bi-fi-ca-tion", "SYL-LA-BI-FI-CA-TION"], "min_len2_1": ["hel-lo"], "min_len2_2": ["hello"],
            "min_len2_5": ["hello", "syllabi-fi-cation"]}.get(name, [])
    assert want[:len(told)] == told                           # the rows of the issue's table
    h = H.bft_load(wc.make_variant(name, tmp_path).encode())
    n, out, off = host_batch(H, h, words, 0x2D)
    same_texts(out, off, want, words, "host build, variant " + name)
    H.bft_free(VP(h))


def test_2_host_tokenizer_model_has_no_hyphenator(H):
    h = H.bft_load(bfutil.model_path("wbd.bin").encode())
    assert H.bft_w2h_ready(VP(h)) == 0 and H.bft_w2h_one(VP(h), b"hyphenation", 11, None, 0, 0x2D) == -1
    assert host_batch(H, h, [b"hyphenation"], 0x2D)[0] == E_UNSUPPORTED
    H.bft_free(VP(h))


# ------------------------------------------------------------------------------------------------
# the product library (GPU tier)
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def L():
    import blingfire_amd as bf
    return bf.lib()


@pytest.fixture(scope="module")
def hmodel():
    import blingfire_amd as bf
    h = bf.load_model(wc.FIXTURE)
    yield h
    bf.free_model(h)


def w2h_case(L, h, words, want, hy, idx=None, what=""):
    from test_gpu_secondary_at_scale import Case
    flat, off = sc.pack(words)
    w_flat, w_off = wc.pack_texts(want)
    if idx is not None:
        flat, off = sc.tile(flat, off, idx)
        w_flat, w_off = sc.tile(w_flat, w_off, idx)
    n = len(off) - 1
    return Case("WordHyphenation %s uHy=0x%x, %d words" % (what, hy, n), L.WordHyphenationBatch, L.WordHyphenationBatchDevice, [VP(h), flat, off, n], [hy], n,
                w_flat, w_off, (flat, off), total_bytes=int(off[-1]))


@pytest.mark.gpu
def test_3_single_call_table(L, hmodel):
    rows = wc.table_rows()
    want = wc.ref_singles("table", wc.FIXTURE, rows)
    for (w, hy, cap), exp in zip(rows, want):
        assert wc.single(L.WordHyphenationWithModel, hmodel, w, hy, cap) == exp, (w[:40], hex(hy), cap)
    # the rows the issue spells out
    by = {(w, hy, cap): exp for (w, hy, cap), exp in zip(rows, want)}
    assert by[(b"syllabification", 0x2D, wc.CAP)] == [21, "syl-la-bi-fi-ca-tion\0"] and by[(b"SYLLABIFICATION", 0x2D, wc.CAP)] == [19, "SYLLABI-FICATI-O-N\0"]
    assert by[(b"syllabification", 0x2D, 10)] == [20, "syl-la-bi-"] and by[(b"x" * 299 + b"\xff", 0x2D, wc.CAP)][0] == -1 and by[(b"x" * 300 + b"\xff", 0x2D, wc.CAP)][0] == 301
    # NULL output pointer: the size, no terminator counted
    for w, hy, cap in rows:
        r = wc.single(L.WordHyphenationWithModel, hmodel, w, hy, cap, null=True)[0]
        exp = by[(w, hy, cap)][0]
        assert r == (exp - 1 if exp > 0 and exp <= cap else exp), (w[:40], hex(hy), r, exp)
    assert L.WordHyphenationWithModel(None, 5, None, 0, VP(hmodel), 0x2D) == -1 and L.WordHyphenationWithModel(b"abc", -1, None, 0, VP(hmodel), 0x2D) == -1


@pytest.mark.gpu
def test_3_single_call_every_capacity(L, hmodel):
    rows = capacity_rows()
    want = wc.ref_singles("capacities", wc.FIXTURE, rows)
    _full_need(want, rows)
    for (w, hy, cap), exp in zip(rows, want):
        assert wc.single(L.WordHyphenationWithModel, hmodel, w, hy, cap) == exp, (w, hex(hy), cap)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["en", "en_upper", "en_capitalised", "corpus"])
def test_4_batch_host_and_device(L, hmodel, name):
    words = wc.batch_lists()[name]
    want = wc.ref_texts("batch_" + name, wc.FIXTURE, words)["45"]
    w2h_case(L, hmodel, words, want, 0x2D, what=name).check(capacity=False)


@pytest.mark.gpu
@pytest.mark.parametrize("hy", wc.UHYS)
def test_4_5_edge_words(L, hmodel, hy):
    named = wc.edge_words()
    words = [w for _, w in named]
    want = wc.ref_texts("edge", wc.FIXTURE, words, wc.UHYS)[str(hy)]
    case = w2h_case(L, hmodel, words, want, hy, what="edge words")
    case.names = [n for n, _ in named]
    case.check()
    for (name, w), t in zip(named, want):                      # ... and the single call on each
        r, s = wc.single(L.WordHyphenationWithModel, hmodel, w, hy, 8 * len(w) + 16)
        assert (s[:r - 1] if r > 0 else "") == t and (r > 0 or r == (0 if not w else -1)), (name, r)


@pytest.mark.gpu
def test_5_hyphens_that_cannot_be_encoded(L, hmodel):
    import torch
    words = [b"syllabification", b"a"]
    flat, off = sc.pack(words)
    out, o_off = np.full(64, 0xA5, dtype=np.uint8), np.full(3, -1, dtype=np.int64)
    d_flat, d_off = torch.from_numpy(flat).cuda(), torch.from_numpy(off).cuda()
    d_out, d_ooff = torch.full((64,), 0xA5, dtype=torch.uint8, device="cuda"), torch.full((3,), -1, dtype=torch.int64, device="cuda")
    for hy in wc.BAD_UHYS:
        assert L.WordHyphenationBatch(VP(hmodel), flat.ctypes.data, off.ctypes.data, 2, out.ctypes.data, 64, o_off.ctypes.data, hy) == E_ARG
        assert L.WordHyphenationBatchDevice(VP(hmodel), d_flat.data_ptr(), d_off.data_ptr(), 2, int(off[-1]), d_out.data_ptr(), 64, d_ooff.data_ptr(), hy, None) == E_ARG
        assert L.WordHyphenationWithModel(words[0], len(words[0]), None, 0, VP(hmodel), hy) == -1
    torch.cuda.synchronize()
    assert (out == 0xA5).all() and (d_out.cpu().numpy() == 0xA5).all()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(wc.VARIANTS))
def test_6_model_variants(L, name, tmp_path):
    import blingfire_amd as bf
    words = wc.variant_words()
    path = wc.make_variant(name, tmp_path)
    want = variant_answers(name, path)
    assert want != wc.ref_texts("variant_base", wc.FIXTURE, words)["45"], "the variant %s exercises nothing on these words" % name
    h = bf.load_model(path)
    try:
        assert L.BfModelKind(VP(h)) == 6
        w2h_case(L, h, words, want, 0x2D, what="variant " + name).check(capacity=False)
    finally:
        bf.free_model(h)


@pytest.mark.gpu
def test_6_refused_models(L, tmp_path):
    for path, word in [(wc.make_variant("unknown_parameter", tmp_path), b"unknown parameter"), (wc.make_variant("zero_anchor", tmp_path), b"left-anchor"),
                       (wc.make_variant("min_len_0", tmp_path), b"min-len"), (wc.make_bad_pattern_value(tmp_path), b"holds the value -1")]:
        assert not L.LoadModel(path.encode())
        assert word in L.BfLastError(), (path, L.BfLastError())


@pytest.mark.gpu
def test_7_at_scale(L, hmodel):
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    en, edge = wc.en_words(), [w for _, w in wc.edge_words()]
    words = en + edge
    want = wc.ref_texts("batch_en", wc.FIXTURE, en)["45"] + wc.ref_texts("edge", wc.FIXTURE, edge, wc.UHYS)["45"]
    if len(words) % 2 == 0:                                    # (sc.tiling wants an odd period)
        words, want = words[:-1], want[:-1]
    assert L.BfReserve(VP(hmodel), 300007, 8 << 20, 0) == 0
    for n, seed in ((3 * 64 * cus + 17, 61), (300007, 67)):
        w2h_case(L, hmodel, words, want, 0x2D, sc.tiling(len(words), n, seed), what="tiled").check(capacity=False)
    # capacity contracts of both forms (the canary tail of 4,096 items), a side stream among the short capacities
    small = w2h_case(L, hmodel, words, want, 0x2D, sc.tiling(len(words), 4099, 71), what="tiled")
    small.check()
    # ... and a full-size call behind them on the same handle: no stale state
    rc, out, off, _ = small.run_dev(small.T)
    assert rc == 0
    small._offsets(off, "Device, after short capacities")
    small._exact(out, off, small.T, "Device, after short capacities")
    small._untouched(out, small.T, "Device, after short capacities")
    tiny = w2h_case(L, hmodel, words[:17], want[:17], 0x2D, what="a second, smaller batch")
    tiny.check()
    assert L.BfLastStatus(VP(hmodel)) == 0
    ms = (ctypes.c_float * 6)()
    assert L.BfLastKernelMs(VP(hmodel), ms, 6) == 6 and ms[4] > 0


@pytest.mark.gpu
def test_7_word_offsets_out_of_range(L, hmodel):
    flat, off = sc.pack([b"syllable", b"hyphen", b"pattern"])
    off = off.copy()
    off[2] = 400                                                # word 1 ends, word 2 begins outside the text: both are empty
    r, s = wc.single(L.WordHyphenationWithModel, hmodel, b"syllable", 0x2D)
    first = s[:r - 1].encode("latin-1")
    assert len(first) > 8
    o_off = np.full(4, -1, dtype=np.int64)
    out = np.full(64, 0xA5, dtype=np.uint8)
    n = L.WordHyphenationBatch(VP(hmodel), flat.ctypes.data, off.ctypes.data, 3, out.ctypes.data, 64, o_off.ctypes.data, 0x2D)
    assert n == len(first) and out[:n].tobytes() == first and (out[n:] == 0xA5).all()
    assert o_off.tolist() == [0, n, n, n]
    assert L.BfLastStatus(VP(hmodel)) & 8


@pytest.mark.gpu
def test_8_other_handles(L, hmodel):
    import blingfire_amd as bf
    h = bf.load_model(bfutil.model_path("wbd.bin"))
    try:
        assert L.WordHyphenationWithModel(b"hyphenation", 11, None, 0, VP(h), 0x2D) == -1
        assert L.WordHyphenationWithModel(b"", 0, None, 0, VP(h), 0x2D) == 0
        flat, off = sc.pack([b"hyphenation"])
        o_off = np.zeros(2, dtype=np.int64)
        assert L.WordHyphenationBatch(VP(h), flat.ctypes.data, off.ctypes.data, 1, None, 0, o_off.ctypes.data, 0x2D) == E_UNSUPPORTED
        assert L.WordHyphenationBatchDevice(VP(h), None, None, 0, 0, None, 0, None, 0x2D, None) == E_UNSUPPORTED
    finally:
        bf.free_model(h)
    ids = (ctypes.c_int32 * 8)()
    assert L.TextToIds(VP(hmodel), b"hyphenation", 11, ids, 8, 0) == 0
    assert L.BfModelKind(VP(hmodel)) == 6
    assert bf.word_hyphenation_with_model(hmodel, "syllabification") == "syl-la-bi-fi-ca-tion"
    assert bf.word_hyphenation_batch(hmodel, ["syllabification", "", "разбивка", b"\xff"], 0x2581) == ["syl▁la▁bi▁fi▁ca▁tion", "", "раз▁бивка", ""]
