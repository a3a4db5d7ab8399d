"""GPU: batches of very many tiny documents (tests/tiny_cases.py) through the C-ABI against the CPU checker (the compiled reference where oracle/_ref is
built, else the oracle) -- EVERY document, ids and byte offsets, bit for bit.

The tokenising kernels are wave programs: one wave opens document after document and carries its table of eight open documents, the 8-bit entry number of
every queued token (bf_wave_body.h / bf_bpe_wave_body.h: (curk & 0xFF) << 16, rebuilt by settle() as dt_head + ((entry - dt_head) & 0xFF)) and its ring base
from one to the next.  Only a document that is really opened takes an entry, so the entry number of a wave wraps once it has opened more than 256 documents.
Each wave-program case therefore asserts, from the checker's answer alone, that `live` -- the documents with at least one id, which certainly took an entry --
exceeds 256 x (an upper bound on the waves the launch code starts): by pigeonhole some wave then opened more than 256 documents.  The bounds:

  launch_wp_wave (bf_kernels.hip): blocks = min(cus * per_cu, ceil(ndocs / (4 * grab))), four waves a block; BfSetVariant bits 24..29 = per_cu (the
      override), bits 12..15 = grab.  With bits 24..29 = 1 at most 4 * cus waves run.  The LIST instance (the documents the flat program hands back) gets no
      override (enqueue_flat sets its WpWaveKnobs::per_cu to 0) and takes what the occupancy query answers: at most the hardware's 32 waves per CU.
  launch_bpe_wave_cfg (bf_kernels_sp.hip): blocks = min(cus * per_cu, ...) with per_cu from the occupancy query, no override: at most 32 waves per CU.

The flat program (batches of >= 1,024 documents and >= 1 MiB on a fresh handle: bf_capi.cpp use_flat) sees chunks of 512 bytes that hold more than 512
documents, the _sp prologue (eight bytes per lane) batches without one document that long, every family a batch without a byte, and the mapped small path
(run_host_mapped: at most 256 documents and 64 KiB) both of its limits.  Sizes follow the device's CU count; every case prints ndocs, live, its wave bound
and the program that ran (pytest -s shows them)."""
import ctypes

import numpy as np
import pytest

import bfutil
import blingfire_amd as bf
import tiny_cases

pytestmark = pytest.mark.gpu

WP_MODELS = [m for m in ("bert_base_tok.bin", "bert_base_cased_tok.bin", "bert_chinese.bin") if bfutil.have_model(m)]
BPE_MODELS = [m for m in ("gpt2.bin", "roberta.bin", "bpe_example.bin", "bpe_example2.bin") if bfutil.have_model(m)]
UNI_MODELS = [m for m in ("xlm_roberta_base.bin", "xlnet.bin", "laser100k.bin") if bfutil.have_model(m)]
OFFSETS_NAME = "TextToIdsWithOffsets" if bfutil.have_ref() else "bfo_text_to_ids_with_offsets"
WP_PAIRS = ((512, 100), (1, 7))                 # (max_ids, unk): everything, and one id per document
SP_PAIRS = ((2048, 0), (1, 1))
LIVE_SHARE = 0.66                               # sizing only: about 0.69 (WordPiece) to 0.85 (BPE) of queries() have an id; every case ASSERTS its condition
SMALL_MAX_DOCS, SMALL_MAX_BYTES = 256, 64 * 1024                   # bf_capi.cpp
BF_E_CAPACITY = -3


@pytest.fixture(scope="module")
def cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


# ------------------------------------------------------------------------------------------------
# inputs and the checker's answers: built once per module, shared, never changed
# ------------------------------------------------------------------------------------------------
_batches, _want_ids, _tables, _ck = {}, {}, {}, {}


def batch_of(key):
    """key: ("queries" | "ones" | "empties" | "giant", n) -> (text, doc_off, index into tiny_cases.table() or None); "giant": with_giant(queries(n))"""
    if key not in _batches:
        kind, n = key
        index = None
        if kind == "giant":
            text, off = tiny_cases.with_giant(batch_of(("queries", n))[:2])
        else:
            text, off = getattr(tiny_cases, kind)(n)
            if kind != "empties":
                index = getattr(tiny_cases, kind + "_index")(n)
                index.flags.writeable = False
        text.flags.writeable = False; off.flags.writeable = False
        _batches[key] = (text, off, index)
    return _batches[key]


def checker(model, no_dummy_prefix=False):
    if "lib" not in _ck:
        _ck["lib"] = bfutil.reference() if bfutil.have_ref() else bfutil.oracle()
    k = (model, no_dummy_prefix)
    if k not in _ck:
        _ck[k] = _ck["lib"].load(bfutil.model_path(model))
        if no_dummy_prefix:
            setter = getattr(_ck["lib"].lib, "SetNoDummyPrefix", None) or getattr(_ck["lib"].lib, "bfo_set_no_dummy_prefix")
            setter.argtypes = [ctypes.c_void_p, ctypes.c_int]
            setter(ctypes.c_void_p(_ck[k]), 1)
    return _ck["lib"], _ck[k]


@pytest.fixture(scope="module", autouse=True)
def _free_checker():
    yield
    for k in [k for k in _ck if k != "lib"]:
        _ck["lib"].free(_ck.pop(k))


def table_answers(model, mx, unk, offsets, no_dummy_prefix=False):
    """the checker's answer for every distinct document (documents are independent): (ids, [first bytes, last bytes,] offsets int64[ndistinct + 1])"""
    key = (model, mx, unk, offsets, no_dummy_prefix)
    if key not in _tables:
        ck, hck = checker(model, no_dummy_prefix)
        docs = tiny_cases.table()[0]
        if offsets:
            wi, ws, we = [], [], []
            ido = np.zeros(len(docs) + 1, dtype=np.int64)
            for d, b in enumerate(docs):
                # (a document of n bytes has at most 2 * (n + 1) ids: asking for no more gives the same answer without three arrays of mx entries per call)
                c, i_, s_, e_ = ck.with_offsets(hck, b, min(mx, 2 * len(b) + 2), unk, OFFSETS_NAME)
                c = min(len(i_), mx)
                wi += i_[:c]; ws += s_[:c]; we += e_[:c]
                ido[d + 1] = ido[d] + c
            out = (np.array(wi, dtype=np.int32), np.array(ws, dtype=np.int32), np.array(we, dtype=np.int32), ido)
        else:
            text, off = bf.pack_docs(docs)
            out = ck.batch(hck, text, off, mx, unk)
        _tables[key] = out
    return _tables[key]


def expanded(key, ans):
    tab_off = ans[-1]
    index = batch_of(key)[2]
    start, length = tab_off[:-1], np.diff(tab_off)
    cols = [tiny_cases.expand(a, start, length, index) for a in ans[:-1]]
    return [c[0] for c in cols] + [cols[0][1]]


def want_ids(model, key, mx, unk, no_dummy_prefix=False):
    """TextToIds of the checker for every document: (ids, id offsets).  The whole batch through bfutil.cpu_ids_compact on host threads; with
    SetNoDummyPrefix, which that driver cannot switch, the per-document answers of the distinct documents, expanded"""
    k = (model, key, mx, unk, no_dummy_prefix)
    if k not in _want_ids:
        text, off, _ = batch_of(key)
        if no_dummy_prefix:
            ids, ido = expanded(key, table_answers(model, mx, unk, False, True))
        else:
            _, ids, ido = bfutil.cpu_ids_compact(bfutil.checker_lib_path()[0], bfutil.model_path(model), text, off, mx, unk)
        ids.flags.writeable = False; ido.flags.writeable = False
        _want_ids[k] = (ids, ido)
    return _want_ids[k]


def want_offsets(model, key, mx, unk):
    """TextToIdsWithOffsets of the checker for every document, from its per-document call memoised by distinct document: (ids, first bytes, last bytes, id offsets)"""
    out = expanded(key, table_answers(model, mx, unk, True))
    wids, woff = want_ids(model, key, mx, unk)
    assert np.array_equal(out[3], woff) and np.array_equal(out[0], wids), "the checker's TextToIdsWithOffsets and TextToIds disagree"
    return out


def live_of(model, key, mx, unk):
    return int((np.diff(want_ids(model, key, mx, unk)[1]) > 0).sum())


# ------------------------------------------------------------------------------------------------
# comparison: whole arrays (every document); on a difference, the first document that differs
# ------------------------------------------------------------------------------------------------
def same(ctx, key, got_off, want_off, pairs):
    """pairs: (what, got array, wanted array) parallel to the id offsets"""
    got_off = np.asarray(got_off)
    if np.array_equal(got_off, want_off) and all(np.array_equal(g, w) for _, g, w in pairs):
        return
    text, off, _ = batch_of(key)
    nd = len(off) - 1
    assert len(got_off) == nd + 1, (ctx, "id offsets of", len(got_off) - 1, "documents for", nd)
    bad = np.flatnonzero(np.diff(got_off) != np.diff(want_off))
    d = int(bad[0]) if len(bad) else nd                      # up to document d both offset arrays agree
    m = int(want_off[d])
    what0 = "id count"
    for what, g, w in pairs:
        diff = np.flatnonzero(g[:m] != w[:m])
        if len(diff):
            dd = int(np.searchsorted(want_off, diff[0], side="right") - 1)
            if dd < d:
                d, what0 = dd, what
    if d == nd:
        raise AssertionError("%s, %s: the arrays differ behind the last document" % (ctx, key))
    what, g, w = next(p for p in pairs if p[0] == what0) if what0 != "id count" else pairs[0]
    a, b = g[got_off[d]:got_off[d + 1]], w[want_off[d]:want_off[d + 1]]
    raise AssertionError("%s, %s: document %d of %d (%d bytes) %r: %s gpu (%d) %s != checker (%d) %s" % (
        ctx, key, d, nd, off[d + 1] - off[d], bytes(text[off[d]:off[d + 1]][:80]), what0, len(a), a[:40].tolist(), len(b), b[:40].tolist()))


def kernel_of(h):
    L = bf.lib()
    L.BfTokeniseKernel.restype = ctypes.c_char_p
    L.BfTokeniseKernel.argtypes = [ctypes.c_void_p]
    return L.BfTokeniseKernel(ctypes.c_void_p(h))


def ran(h, ctx, kernel):
    assert bf.lib().BfLastStatus(ctypes.c_void_p(h)) == 0, ctx
    if kernel is not None:
        assert kernel_of(h) == kernel, (ctx, kernel_of(h))


def set_variant(h, variant):
    assert bf.lib().BfSetVariant(ctypes.c_void_p(h), variant) >= 0, "BfSetVariant refused %#x" % variant


def run_ids(h, model, key, variant, mx, unk, kernel, no_dummy_prefix=False):
    text, off, _ = batch_of(key)
    ids, id_off = bf.text_to_ids_batch(h, (text, off), mx, unk)
    ctx = "%s variant %s max_ids %d unk %d TextToIdsBatch" % (model, variant, mx, unk)
    ran(h, ctx, kernel)
    wids, woff = want_ids(model, key, mx, unk, no_dummy_prefix)
    same(ctx, key, id_off, woff, [("ids", ids, wids)])
    return ids, id_off


def run_offsets(h, model, key, variant, mx, unk, kernel=None):
    text, off, _ = batch_of(key)
    ids, st, en, id_off = bf.text_to_ids_with_offsets_batch(h, (text, off), mx, unk)
    ctx = "%s variant %s max_ids %d unk %d TextToIdsWithOffsetsBatch" % (model, variant, mx, unk)
    assert bf.lib().BfLastStatus(ctypes.c_void_p(h)) == 0, ctx
    if kernel is not None:
        assert kernel_of(h) == kernel, (ctx, kernel_of(h))
    wids, ws, we, woff = want_offsets(model, key, mx, unk)
    same(ctx, key, id_off, woff, [("ids", ids, wids), ("first bytes", st, ws), ("last bytes", en, we)])
    return ids, st, en, id_off


def run_device(h, model, key, cap, mx, unk, offsets, kernel, tail=64):
    """TextToIdsBatchDevice / TextToIdsWithOffsetsBatchDevice with ids_cap == cap into arrays `tail` entries longer that hold a sentinel: everything arrives,
    nothing at or behind the cap is written.  A batch without a byte passes a 1-byte dummy allocation as d_text"""
    import torch
    text, off, _ = batch_of(key)
    nd = len(off) - 1
    dev = torch.device("cuda", 0)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    dt = torch.from_numpy(text.copy()).to(dev) if len(text) else torch.zeros(1, dtype=torch.uint8, device=dev)
    do = torch.from_numpy(off.copy()).to(dev)
    out, sts, ens = (torch.full((cap + tail,), -7, dtype=torch.int32, device=dev) for _ in range(3))
    ido = torch.full((nd + 1,), -7, dtype=torch.int64, device=dev)
    if offsets:
        what = "TextToIdsWithOffsetsBatchDevice"
        r = bf.lib().TextToIdsWithOffsetsBatchDevice(ctypes.c_void_p(h), dt.data_ptr(), do.data_ptr(), nd, len(text), out.data_ptr(), sts.data_ptr(), ens.data_ptr(), cap,
                                                     ido.data_ptr(), mx, unk, stream)
    else:
        what = "TextToIdsBatchDevice"
        r = bf.lib().TextToIdsBatchDevice(ctypes.c_void_p(h), dt.data_ptr(), do.data_ptr(), nd, len(text), out.data_ptr(), cap, ido.data_ptr(), mx, unk, stream)
    ctx = "%s max_ids %d unk %d %s ids_cap %d" % (model, mx, unk, what, cap)
    assert r == 0, (ctx, r)
    torch.cuda.synchronize(dev)
    ran(h, ctx, kernel)
    g, gs, ge, goff = out.cpu().numpy(), sts.cpu().numpy(), ens.cpu().numpy(), ido.cpu().numpy()
    n = int(goff[-1])
    assert 0 <= n <= cap and (g[n:] == -7).all() and (gs[n if offsets else 0:] == -7).all() and (ge[n if offsets else 0:] == -7).all(), ctx
    if offsets:
        wids, ws, we, woff = want_offsets(model, key, mx, unk)
        same(ctx, key, goff, woff, [("ids", g[:n], wids), ("first bytes", gs[:n], ws), ("last bytes", ge[:n], we)])
    else:
        wids, woff = want_ids(model, key, mx, unk)
        same(ctx, key, goff, woff, [("ids", g[:n], wids)])


def report(case, model, key, live, bound, program):
    nd = len(batch_of(key)[1]) - 1
    print("case %s %s %s: ndocs %d, live %d, wave bound %s, program %s" % (case, model, key, nd, live, bound, program.decode() if isinstance(program, bytes) else program))


def n_for_live(want_live):
    return int(want_live / LIVE_SHARE) + 1


# ------------------------------------------------------------------------------------------------
# a. the WordPiece wave program, long-lived waves
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", WP_MODELS)
def test_a_wordpiece_waves_open_more_than_256_documents(model, cus):
    """variant 5 | (1 << 24) | (g << 12): never the flat program, one workgroup = four waves per CU (launch_wp_wave's per_cu_override), g documents per grab:
    at most 4 * cus waves, and live > 256 * 4 * cus.  Ids at g = 1, 3, 8, ids with offsets (the OFFS instance) at g = 8, and the lane-per-document kernels
    (variant 2) once as the cross-check the other parity modules keep"""
    key = ("queries", n_for_live(1.3 * 1024 * cus))
    waves = 4 * cus
    h = bf.load_model(bfutil.model_path(model))
    try:
        for mx, unk in WP_PAIRS:
            live = live_of(model, key, mx, unk)
            assert live > 256 * waves, (model, key, live, waves)
        report("a", model, key, live, waves, "k_wp_wave")
        for g in (1, 3, 8):
            variant = 5 | (1 << 24) | (g << 12)
            set_variant(h, variant)
            for mx, unk in WP_PAIRS:
                run_ids(h, model, key, hex(variant), mx, unk, b"k_wp_wave")
                if g == 8:
                    run_offsets(h, model, key, hex(variant), mx, unk, b"k_wp_wave")
        set_variant(h, 2)
        ids, id_off = bf.text_to_ids_batch(h, batch_of(key)[:2], 512, 100)
        assert bf.lib().BfLastStatus(ctypes.c_void_p(h)) == 0 and kernel_of(h) in (b"k_lex_wp_flat", b"k_lex_wp_plain")
        wids, woff = want_ids(model, key, 512, 100)
        same(model + " variant 2", key, id_off, woff, [("ids", ids, wids)])
    finally:
        bf.free_model(h)


# ------------------------------------------------------------------------------------------------
# b. the wave program chosen by itself: eight documents per grab by the launch rule
# ------------------------------------------------------------------------------------------------
def key_b(cus):
    return ("queries", 8 * 32 * cus + 77)


def assert_b(key, cus):
    text, off, _ = batch_of(key)
    nd = len(off) - 1
    assert len(text) < 1 << 20                               # (use_flat: under 1 MiB the batch stays off the flat program)
    assert nd // (cus * 32) >= 8                             # (launch_wp_wave: grab = min(ndocs / (cus * 32), WV_GRAB_MAX = 8))


@pytest.mark.parametrize("model", WP_MODELS)
def test_b_wave_program_by_itself_grabs_eight(model, cus):
    """a fresh handle, the default variant: the host form, TextToIdsBatchDevice and TextToIdsWithOffsetsBatchDevice with ids_cap == the exact total"""
    key = key_b(cus)
    assert_b(key, cus)
    mx, unk = WP_PAIRS[0]
    h = bf.load_model(bfutil.model_path(model))
    try:
        run_ids(h, model, key, "default", mx, unk, b"k_wp_wave")
        nd = len(batch_of(key)[1]) - 1
        report("b", model, key, live_of(model, key, mx, unk), "min(4 * cus * per_cu, 4 * ceil(%d / 32)), grab 8" % nd, kernel_of(h))
        cap = int(want_ids(model, key, mx, unk)[1][-1])
        assert cap > 0
        run_device(h, model, key, cap, mx, unk, False, b"k_wp_wave")
        run_device(h, model, key, cap, mx, unk, True, b"k_wp_wave")
    finally:
        bf.free_model(h)


# ------------------------------------------------------------------------------------------------
# c. the flat program chosen by itself, dense with documents
# ------------------------------------------------------------------------------------------------
KEYS_C = {"ones": ("ones", (1 << 20) + 4096), "queries": ("queries", 250000)}


@pytest.mark.parametrize("name", list(KEYS_C))
@pytest.mark.parametrize("model", WP_MODELS)
def test_c_flat_program_by_itself_dense_with_documents(model, name, cus):
    """chunks of 512 bytes with hundreds of documents (ones(): more documents than bytes), k_wp_count / k_wp_merge blocks of 64 documents that are all empty;
    then the same handle runs case b's batch and this batch once more: nothing of a 10^6-document batch stays in dstat, counts or the word records"""
    key = KEYS_C[name]
    text, off, _ = batch_of(key)
    assert len(off) - 1 >= 1024 and len(text) >= 1 << 20     # (use_flat)
    if name == "ones":
        assert len(text) >= (1 << 20) + 4096
    h = bf.load_model(bfutil.model_path(model))
    try:
        first = None
        for mx, unk in WP_PAIRS:
            got = run_ids(h, model, key, "default", mx, unk, b"k_wp_flat")
            first = first or got
            run_offsets(h, model, key, "default", mx, unk, b"k_wp_flat")
        report("c", model, key, live_of(model, key, *WP_PAIRS[0]), "- (ranges of bytes, not documents)", kernel_of(h))
        kb = key_b(cus)
        assert_b(kb, cus)
        run_ids(h, model, kb, "default", *WP_PAIRS[0], b"k_wp_wave")
        last = run_ids(h, model, key, "default", *WP_PAIRS[0], b"k_wp_flat")
        assert first[0].tobytes() == last[0].tobytes() and first[1].tobytes() == last[1].tobytes()
    finally:
        bf.free_model(h)


# ------------------------------------------------------------------------------------------------
# d. everything handed back to the wave program's LIST instance
# ------------------------------------------------------------------------------------------------
def n_de(cus):
    return n_for_live(1.02 * 256 * 32 * cus)


def test_d_everything_handed_back(cus):
    """one document of WF_DOC_MAX + 5 bytes: k_wp_pre calls the batch unfit, k_wp_hardlist lists every document, k_wp_wave<..., LIST> (grab 1, a full grid whatever
    BfSetVariant says: at most 32 waves per CU) tokenises all of them"""
    model = "bert_base_tok.bin" if bfutil.have_model("bert_base_tok.bin") else bfutil.bert_model_name()
    key = ("giant", n_de(cus))
    mx, unk = 1 << 22, 100
    waves = 32 * cus
    live = live_of(model, key, mx, unk)
    assert live > 256 * waves, (model, key, live, waves)
    h = bf.load_model(bfutil.model_path(model))
    try:
        run_ids(h, model, key, "default", mx, unk, b"k_wp_flat")
        report("d", model, key, live, waves, "k_wp_flat -> k_wp_wave<LIST> (unfit batch)")
    finally:
        bf.free_model(h)


# ------------------------------------------------------------------------------------------------
# e. BPE
# ------------------------------------------------------------------------------------------------
def assert_safe_cap(model, key, mx, unk):
    """the header's bound for ids_cap that is safe for any input: 2 * (total_bytes + ndocs).  Tiny documents are where it is tightest"""
    text, off, _ = batch_of(key)
    cap = 2 * (len(text) + len(off) - 1)
    total = int(want_ids(model, key, mx, unk)[1][-1])
    assert total <= cap, (model, key, total, cap)
    return cap


@pytest.mark.parametrize("model", BPE_MODELS)
def test_e_bpe_waves_open_more_than_256_documents(model, cus):
    """the batch of case d without the giant: launch_bpe_wave_cfg has no override, so live > 256 * 32 * cus whatever the occupancy query answers.  The shipped
    HOME form (3), the in-order form (3 | 8 << 8) and the lane kernels alone with their dynamic refill (3 | 0x40)"""
    key = ("queries", n_de(cus))
    waves = 32 * cus
    L = bf.lib()
    L.BfBpeFallbackDocs.restype = ctypes.c_longlong; L.BfBpeFallbackDocs.argtypes = [ctypes.c_void_p]
    h = bf.load_model(bfutil.model_path(model))
    try:
        for mx, unk in SP_PAIRS:
            live = live_of(model, key, mx, unk)
            assert live > 256 * waves, (model, key, live, waves)
            assert_safe_cap(model, key, mx, unk)
        for variant, kernel in ((3, b"k_bpe_wave"), (3 | (8 << 8), b"k_bpe_wave"), (3 | 0x40, b"k_bpe_fused")):
            set_variant(h, variant)
            for mx, unk in SP_PAIRS:
                run_ids(h, model, key, hex(variant), mx, unk, kernel)
                print("case e %s variant %#x max_ids %d: BfBpeFallbackDocs %d" % (model, variant, mx, L.BfBpeFallbackDocs(ctypes.c_void_p(h))))
            report("e", model, key, live, waves, kernel)
        set_variant(h, 3)
        small = ("queries", 1024 * cus)
        mx, unk = SP_PAIRS[0]
        run_offsets(h, model, small, 3, mx, unk)
        run_device(h, model, small, assert_safe_cap(model, small, mx, unk), mx, unk, False, b"k_bpe_wave")
    finally:
        bf.free_model(h)


# ------------------------------------------------------------------------------------------------
# f. Unigram: the _sp prologue (eight bytes per lane) on documents that are all shorter than that
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["queries", "ones"])
@pytest.mark.parametrize("model", UNI_MODELS)
def test_f_unigram_tiny_documents(model, name, cus):
    """the cut form (3), the forward / backward kernels (6) and the byte-per-lane prologue (3 | 0x80): ids and offsets; SetNoDummyPrefix on and off for xlnet.bin;
    TextToIdsBatchDevice with exactly the header's safe ids_cap, 2 * (total_bytes + ndocs) -- a dummy prefix per one-byte document is where it is tightest"""
    key = (name, 1024 * cus)
    h = bf.load_model(bfutil.model_path(model))
    try:
        for mx, unk in SP_PAIRS:
            assert_safe_cap(model, key, mx, unk)
        for variant, kernel in ((3, b"k_uni_cut"), (6, b"k_seg_unigram_lane"), (3 | 0x80, b"k_uni_cut")):
            set_variant(h, variant)
            for mx, unk in SP_PAIRS:
                run_ids(h, model, key, hex(variant), mx, unk, kernel)
            if variant != 6:                                 # (the offsets API takes the forward / backward kernels under every variant: the prologue is what differs)
                run_offsets(h, model, key, hex(variant), *SP_PAIRS[0])
        report("f", model, key, live_of(model, key, *SP_PAIRS[0]), "- (lane programs)", b"k_uni_cut, k_seg_unigram_lane")
        set_variant(h, 3)
        mx, unk = SP_PAIRS[0]
        run_device(h, model, key, assert_safe_cap(model, key, mx, unk), mx, unk, False, b"k_uni_cut")
        if model == "xlnet.bin":
            bf.change_settings_dummy_prefix(h, False)
            for variant, kernel in ((3, b"k_uni_cut"), (3 | 0x80, b"k_uni_cut")):
                set_variant(h, variant)
                ids, _ = run_ids(h, model, key, hex(variant) + " no dummy prefix", mx, unk, kernel, no_dummy_prefix=True)
            assert not np.array_equal(ids, want_ids(model, key, mx, unk)[0])
            bf.change_settings_dummy_prefix(h, True)
            set_variant(h, 3)
            run_ids(h, model, key, "3, dummy prefix back", mx, unk, b"k_uni_cut")
    finally:
        bf.free_model(h)


# ------------------------------------------------------------------------------------------------
# g. total_bytes == 0
# ------------------------------------------------------------------------------------------------
FAMILIES = [(m, k, mx, unk) for m, k, (mx, unk) in (("bert_base_tok.bin", b"k_wp_wave", WP_PAIRS[0]), ("gpt2.bin", b"k_bpe_wave", SP_PAIRS[0]),
                                                     ("xlm_roberta_base.bin", b"k_uni_cut", SP_PAIRS[0])) if bfutil.have_model(m)]


@pytest.mark.parametrize("model,kernel,mx,unk", FAMILIES)
def test_g_many_documents_without_a_byte(model, kernel, mx, unk, cus):
    """many empty documents: every count 0, offsets all 0, status 0 -- the host form, the Device form (d_text: a 1-byte dummy allocation) and a handle sharded
    over three ranges (BfSetDevices [0, 0, 0]), which also runs queries(1024 * cus)"""
    key = ("empties", 8 * 32 * cus + 77)
    text, off, _ = batch_of(key)
    nd = len(off) - 1
    h = bf.load_model(bfutil.model_path(model))
    try:
        def empty_host(ctx, want_kernel):
            ids, id_off = bf.text_to_ids_batch(h, (text, off), mx, unk)
            assert len(ids) == 0 and len(id_off) == nd + 1 and not id_off.any(), ctx
            assert bf.lib().BfLastStatus(ctypes.c_void_p(h)) == 0, ctx
            if want_kernel is not None:                  # (asked right after the ids call: the offsets API of a Unigram model takes other kernels)
                assert kernel_of(h) == want_kernel, (ctx, kernel_of(h))
            ids, st, en, id_off = bf.text_to_ids_with_offsets_batch(h, (text, off), mx, unk)
            assert len(ids) == 0 and len(st) == 0 and len(en) == 0 and not id_off.any(), ctx
            assert bf.lib().BfLastStatus(ctypes.c_void_p(h)) == 0, ctx

        wids, woff = want_ids(model, key, mx, unk)
        assert len(wids) == 0 and not woff.any()
        empty_host(model + " host form", kernel)
        run_device(h, model, key, 0, mx, unk, False, kernel)
        run_device(h, model, key, 64, mx, unk, False, kernel, tail=0)
        report("g", model, key, 0, "-", kernel_of(h))
        bf.set_devices(h, [0, 0, 0])
        empty_host(model + " three ranges", None)
        small = ("queries", 1024 * cus)
        run_ids(h, model, small, "default, three ranges", mx, unk, None)          # (which program ran is each range's handle's to say)
    finally:
        bf.free_model(h)


# ------------------------------------------------------------------------------------------------
# h. the mapped small path at its limits
# ------------------------------------------------------------------------------------------------
def small_batches():
    dots = b"." * 256
    return {
        "256 x 256 bytes": [dots] * SMALL_MAX_DOCS,                                          # exactly 65,536 bytes and 65,536 ids: the mapped path
        "one byte more": [dots] * (SMALL_MAX_DOCS - 1) + [dots + b"."],                       # the regular path
        "257 documents": [dots] * SMALL_MAX_DOCS + [b"a"],
        "256 empty": [b""] * SMALL_MAX_DOCS,
        "255 empty, one of 65,536 bytes": [b""] * (SMALL_MAX_DOCS - 1) + [b"." * SMALL_MAX_BYTES],
    }


@pytest.mark.parametrize("variant", [3, 3 | (8 << 12)])
def test_h_mapped_small_path_at_its_limits(variant):
    """run_host_mapped takes at most 256 documents and 64 KiB: the answer on either side of both limits equals the checker's; ids_cap one short is
    BF_E_CAPACITY with complete offsets and not one id written.  3 | (8 << 12): eight documents per wave in round-robin ranges (next_doc == nullptr)"""
    model = bfutil.bert_model_name()
    mx, unk = 1 << 17, 100
    ck, hck = checker(model)
    h = bf.load_model(bfutil.model_path(model))
    try:
        set_variant(h, variant)
        for name, docs in small_batches().items():
            text, off = bf.pack_docs(docs)
            if name == "256 x 256 bytes":
                assert len(docs) == SMALL_MAX_DOCS and len(text) == SMALL_MAX_BYTES
            wids, woff = ck.batch(hck, text, off, mx, unk)
            ids, id_off = bf.text_to_ids_batch(h, (text, off), mx, unk)
            ctx = "%s variant %#x %s" % (model, variant, name)
            assert bf.lib().BfLastStatus(ctypes.c_void_p(h)) == 0 and kernel_of(h) == b"k_wp_wave", ctx
            assert np.array_equal(id_off, woff) and np.array_equal(ids, wids), ctx
            if name == "256 x 256 bytes":
                assert len(wids) == SMALL_MAX_BYTES
                cap = len(wids) - 1
                out = np.full(cap + 64, -7, dtype=np.int32)
                ido = np.full(len(off), -7, dtype=np.int64)
                r = bf.lib().TextToIdsBatch(ctypes.c_void_p(h), text.ctypes.data, off.ctypes.data, len(off) - 1, out.ctypes.data, cap, ido.ctypes.data, mx, unk)
                assert r == BF_E_CAPACITY and np.array_equal(ido, woff) and (out == -7).all(), (ctx, r)
            print("case h %s: ndocs %d, live %d, wave bound -, program %s" % (ctx, len(docs), int((np.diff(woff) > 0).sum()), kernel_of(h).decode()))
    finally:
        bf.free_model(h)
