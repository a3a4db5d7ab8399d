"""GPU parity of the flat WordPiece program (k_wp_pre -> k_wp_flat -> k_wp_units -> k_wp_hardlist -> k_wp_wave<LIST> -> k_wp_count -> scan ->
k_wp_merge) on text it was NOT tuned on: the builders of tests/flat_cases.py at device size, through the C-ABI, against the
CPU checker (the compiled reference where oracle/_ref is built, else the oracle) -- every document, ids and byte offsets, bit for bit.

The metric's corpus hands no document back to the wave program.  Here 1 % (real lines) to about half (multilingual text) of the documents leave the
flat program, so thousands of waves with private record lists, per-document atomics, the shared hard list and the merge of streamed and
handed-back documents in blocks of 64 are what is under test; tests/test_flat_emu.py runs the same builders in the simulator (1 - 3 waves in order).
Every call asserts that the flat program ran (BfTokeniseKernel, BfLastStatus) and the instrumented instances say what it did (BfLexStats)."""
import ctypes

import numpy as np
import pytest

import bfutil
import blingfire_amd as bf
import flat_cases

pytestmark = pytest.mark.gpu

WP_MODELS = [m for m in ("bert_base_tok.bin", "bert_base_cased_tok.bin", "bert_chinese.bin") if bfutil.have_model(m)]
OFFSETS_NAME = "TextToIdsWithOffsets" if bfutil.have_ref() else "bfo_text_to_ids_with_offsets"
PAIRS = ((512, 100), (8, 7))                                   # (max_ids, unk): everything, and a truncating pair
BUILDERS = {
    "real_lines": lambda: flat_cases.real_lines(30000),
    "multilingual": lambda: flat_cases.multilingual(4000),
    "mixture": lambda: flat_cases.mixture(2400),
    "shapes0": lambda: flat_cases.shapes(0, 2000),
    "shapes1": lambda: flat_cases.shapes(1, 2000),
    "shapes2": lambda: flat_cases.shapes(2, 2000),
    "size_limits": lambda: flat_cases.size_limits(400),
}
BY_ITSELF = ("real_lines", "multilingual", "mixture")           # a fresh handle chooses the flat program for these (>= 1,024 documents, >= 1 MiB)
INPUTS = list(BUILDERS)


def pairs_of(name):
    return ((1 << 22, 100), (64, 100)) if name == "size_limits" else PAIRS


# ------------------------------------------------------------------------------------------------
# inputs and the checker's answers: built once, shared by every test of the module, never changed
# ------------------------------------------------------------------------------------------------
_inputs, _ck, _want_ids, _want_offsets = {}, {}, {}, {}


def batch_of(name):
    if name not in _inputs:
        text, off = BUILDERS[name]()
        text.flags.writeable = False; off.flags.writeable = False
        _inputs[name] = (text, off)
    return _inputs[name]


def checker(model):
    if "lib" not in _ck:
        _ck["lib"] = bfutil.reference() if bfutil.have_ref() else bfutil.oracle()
    if model not in _ck:
        _ck[model] = _ck["lib"].load(bfutil.model_path(model))
    return _ck["lib"], _ck[model]


@pytest.fixture(scope="module", autouse=True)
def _free_checker():
    yield
    for model in [k for k in _ck if k != "lib"]:
        _ck["lib"].free(_ck.pop(model))


def want_ids(model, name, mx, unk):
    """TextToIds of the checker per document: (ids, id offsets)"""
    key = (model, name, mx, unk)
    if key not in _want_ids:
        ck, hck = checker(model)
        text, off = batch_of(name)
        ids, id_off = ck.batch(hck, text, off, mx, unk)
        ids.flags.writeable = False; id_off.flags.writeable = False
        _want_ids[key] = (ids, id_off)
    return _want_ids[key]


def want_offsets(model, name, mx, unk):
    """TextToIdsWithOffsets of the checker for EVERY document: (ids, first bytes, last bytes, id offsets)"""
    key = (model, name, mx, unk)
    if key not in _want_offsets:
        ck, hck = checker(model)
        text, off = batch_of(name)
        raw = text.tobytes()
        nd = len(off) - 1
        wi, ws, we = [], [], []
        id_off = np.zeros(nd + 1, dtype=np.int64)
        for d in range(nd):
            b = raw[off[d]:off[d + 1]]
            # (a document of n bytes has at most n ids: asking for min(mx, n + 1) gives the same answer without three arrays of mx entries per call)
            c, i_, s_, e_ = ck.with_offsets(hck, b, min(mx, len(b) + 1), unk, OFFSETS_NAME)
            c = min(len(i_), mx)
            wi.append(np.asarray(i_[:c], dtype=np.int32)); ws.append(np.asarray(s_[:c], dtype=np.int32)); we.append(np.asarray(e_[:c], dtype=np.int32))
            id_off[d + 1] = id_off[d] + c
        out = tuple(np.concatenate(x) if x else np.zeros(0, dtype=np.int32) for x in (wi, ws, we)) + (id_off,)
        for a in out:
            a.flags.writeable = False
        _want_offsets[key] = out
    return _want_offsets[key]


# ------------------------------------------------------------------------------------------------
# comparison: whole arrays (every document); on a difference, the first document that differs
# ------------------------------------------------------------------------------------------------
def same(ctx, name, got_off, want_off, pairs):
    """pairs: (what, got array, wanted array) parallel to the id offsets"""
    if np.array_equal(got_off, want_off) and all(np.array_equal(g, w) for _, g, w in pairs):
        return
    text, off = batch_of(name)
    for d in range(len(off) - 1):
        for what, g, w in pairs:
            a, b = g[got_off[d]:got_off[d + 1]], w[want_off[d]:want_off[d + 1]]
            if not np.array_equal(a, b):
                raise AssertionError("%s, %s: document %d of %d (%d bytes) %r: %s gpu (%d) %s != checker (%d) %s" % (
                    ctx, name, d, len(off) - 1, off[d + 1] - off[d], bytes(text[off[d]:off[d + 1]][:80]), what, len(a), a[:40].tolist(), len(b), b[:40].tolist()))
    raise AssertionError("%s, %s: the id offsets differ behind the last document" % (ctx, name))


def ctx_of(model, variant, mx, unk, step=""):
    return "model %s variant %s max_ids %d unk %d%s" % (model, variant, mx, unk, step and " (" + step + ")")


def flat_ran(h, ctx):
    L = bf.lib()
    L.BfTokeniseKernel.restype = ctypes.c_char_p
    L.BfTokeniseKernel.argtypes = [ctypes.c_void_p]
    assert L.BfTokeniseKernel(ctypes.c_void_p(h)) == b"k_wp_flat", ctx
    assert L.BfLastStatus(ctypes.c_void_p(h)) == 0, ctx


def run_ids(h, model, name, variant, mx, unk, step="", flat=True):
    ids, id_off = bf.text_to_ids_batch(h, batch_of(name), mx, unk)
    ctx = ctx_of(model, variant, mx, unk, step)
    if flat:
        flat_ran(h, ctx)
    wids, woff = want_ids(model, name, mx, unk)
    same(ctx, name, id_off, woff, [("ids", ids, wids)])
    return ids, id_off


def run_offsets(h, model, name, variant, mx, unk, step=""):
    ids, st, en, id_off = bf.text_to_ids_with_offsets_batch(h, batch_of(name), mx, unk)
    ctx = ctx_of(model, variant, mx, unk, step or "offsets")
    flat_ran(h, ctx)
    wids, ws, we, woff = want_offsets(model, name, mx, unk)
    same(ctx, name, id_off, woff, [("ids", ids, wids), ("first bytes", st, ws), ("last bytes", en, we)])


def fresh_handle(model, name):
    """(handle, variant): a fresh handle with the default variant where the batch takes the flat program by itself, BfSetVariant 4 (every batch) elsewhere"""
    h = bf.load_model(bfutil.model_path(model))
    if name in BY_ITSELF:
        return h, "default"
    bf.lib().BfSetVariant(h, 4)
    return h, 4


# ------------------------------------------------------------------------------------------------
# tests
# ------------------------------------------------------------------------------------------------
def test_inputs_are_what_the_flat_program_chooses_by_itself():
    for name in BY_ITSELF:
        text, off = batch_of(name)
        assert len(off) - 1 >= 1024 and len(text) >= 1 << 20, name
    assert len(batch_of("real_lines")[1]) - 1 >= 30000 and len(batch_of("multilingual")[1]) - 1 >= 2100
    text, off = batch_of("mixture")
    assert len(off) - 1 >= 3000 and (np.diff(off) == 0).sum() >= 40
    assert int(np.diff(batch_of("size_limits")[1]).max()) == flat_cases.WF_DOC_MAX
    for r in range(flat_cases.SHAPES_ROTATIONS):
        assert batch_of("shapes%d" % r)[0].tobytes().endswith(flat_cases.TAILS[r])


@pytest.mark.parametrize("name", INPUTS)
@pytest.mark.parametrize("model", WP_MODELS)
def test_ids_and_what_the_program_did(model, name):
    """TextToIdsBatch equals the checker's TextToIds for every document, the flat program ran, and its instrumented instances (BfSetLexStats) say
    that it resolved tokens from the table, that k_wp_units walked words and -- on every input but size_limits -- that documents were handed back"""
    h, variant = fresh_handle(model, name)
    try:
        for mx, unk in pairs_of(name):
            run_ids(h, model, name, variant, mx, unk)
        L = bf.lib()
        L.BfLexStats.restype = ctypes.c_int
        L.BfLexStats.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
        buf = (ctypes.c_ulonglong * 16)()
        L.BfSetLexStats(ctypes.c_void_p(h), 1)
        mx, unk = pairs_of(name)[0]
        run_ids(h, model, name, variant, mx, unk, "the instrumented instances")
        assert L.BfLexStats(ctypes.c_void_p(h), buf, 16) == 16
        L.BfSetLexStats(ctypes.c_void_p(h), 0)
        st = [int(x) for x in buf]
        print("%s %s: chunks %d, tokens %d, table hits %d, words walked by k_wp_units %d, hand-back events %d" % (model, name, st[0], st[2], st[3], st[4], st[7]))
        assert st[3] > 0 and st[4] > 0, (model, name, st)
        if name != "size_limits":
            assert st[7] > 0, (model, name, st)
    finally:
        bf.free_model(h)


@pytest.mark.parametrize("name", INPUTS)
@pytest.mark.parametrize("model", WP_MODELS)
def test_offsets(model, name):
    """TextToIdsWithOffsetsBatch equals the checker's TextToIdsWithOffsets for every document: ids, first bytes, last bytes"""
    h, variant = fresh_handle(model, name)
    try:
        for mx, unk in pairs_of(name):
            run_offsets(h, model, name, variant, mx, unk)
    finally:
        bf.free_model(h)


@pytest.mark.parametrize("name", ["multilingual", "mixture"])
@pytest.mark.parametrize("model", WP_MODELS)
def test_wave_and_lane_programs_on_the_same_text(model, name):
    """the other two roads of a WordPiece batch -- the wave program for every document (variant 5) and the lane-per-document kernels (2) -- give the
    checker's answer on this text as well"""
    h = bf.load_model(bfutil.model_path(model))
    try:
        for variant in (5, 2):
            bf.lib().BfSetVariant(h, variant)
            run_ids(h, model, name, variant, 512, 100, flat=False)
            bf.lib().BfTokeniseKernel.restype = ctypes.c_char_p
            assert bf.lib().BfTokeniseKernel(ctypes.c_void_p(h)) != b"k_wp_flat"
            assert bf.lib().BfLastStatus(ctypes.c_void_p(h)) == 0
    finally:
        bf.free_model(h)


@pytest.mark.parametrize("model", WP_MODELS)
def test_one_handle_many_batches(model):
    """batches of different shapes and calls on ONE handle, workspaces reused: nothing a batch leaves behind (dstat, wrec_cnt, counts, the hard list,
    home cells) reaches the next one; the last step is byte-identical to the first"""
    h = bf.load_model(bfutil.model_path(model))
    ck, hck = checker(model)
    try:
        first = run_ids(h, model, "real_lines", "default", 512, 100, "step 1")
        small = flat_cases.docs_of(batch_of("multilingual"))[:10]
        text, off = bf.pack_docs(small)
        ids, id_off = bf.text_to_ids_batch(h, (text, off), 512, 100)                     # ten documents: the wave program
        bf.lib().BfTokeniseKernel.restype = ctypes.c_char_p
        assert bf.lib().BfTokeniseKernel(ctypes.c_void_p(h)) == b"k_wp_wave"
        wids, woff = ck.batch(hck, text, off, 512, 100)
        assert np.array_equal(id_off, woff) and np.array_equal(ids, wids), (model, "step 2")
        run_offsets(h, model, "multilingual", "default", 512, 100, "step 3, offsets")
        bf.lib().BfSetVariant(h, 4)
        run_ids(h, model, "shapes0", 4, 512, 100, "step 4")
        bf.lib().BfSetVariant(h, 3)                                                      # (3: the default of a fresh handle)
        run_ids(h, model, "multilingual", "default", 8, 7, "step 5")
        last = run_ids(h, model, "real_lines", "default", 512, 100, "step 6")
        assert first[0].tobytes() == last[0].tobytes() and first[1].tobytes() == last[1].tobytes()
    finally:
        bf.free_model(h)


@pytest.mark.parametrize("model", WP_MODELS)
def test_device_form_with_exactly_the_room_needed(model):
    """TextToIdsBatchDevice and TextToIdsWithOffsetsBatchDevice on torch tensors with ids_cap == the ids the batch has: everything arrives, nothing at or
    behind the cap is written (the arrays are 64 entries longer and hold a sentinel)"""
    import torch
    name, mx, unk = "multilingual", 512, 100
    text, off = batch_of(name)
    nd = len(off) - 1
    wids, ws, we, woff = want_offsets(model, name, mx, unk)
    wids0, woff0 = want_ids(model, name, mx, unk)
    cap = int(woff0[-1])
    assert cap == int(woff[-1]) > 0
    h = bf.load_model(bfutil.model_path(model))
    try:
        dev = torch.device("cuda", 0)
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        dt, do = torch.from_numpy(text.copy()).to(dev), torch.from_numpy(off.copy()).to(dev)
        out, sts, ens = (torch.full((cap + 64,), -7, dtype=torch.int32, device=dev) for _ in range(3))
        ido = torch.full((nd + 1,), -7, dtype=torch.int64, device=dev)
        r = bf.lib().TextToIdsBatchDevice(ctypes.c_void_p(h), dt.data_ptr(), do.data_ptr(), nd, len(text), out.data_ptr(), cap, ido.data_ptr(), mx, unk, stream)
        assert r == 0
        torch.cuda.synchronize(dev)
        ctx = ctx_of(model, "default", mx, unk, "TextToIdsBatchDevice")
        flat_ran(h, ctx)
        g = out.cpu().numpy()
        assert (g[cap:] == -7).all(), ctx
        same(ctx, name, ido.cpu().numpy(), woff0, [("ids", g[:cap], wids0)])
        out.fill_(-7); ido.fill_(-7)
        r = bf.lib().TextToIdsWithOffsetsBatchDevice(ctypes.c_void_p(h), dt.data_ptr(), do.data_ptr(), nd, len(text), out.data_ptr(), sts.data_ptr(), ens.data_ptr(), cap,
                                                     ido.data_ptr(), mx, unk, stream)
        assert r == 0
        torch.cuda.synchronize(dev)
        ctx = ctx_of(model, "default", mx, unk, "TextToIdsWithOffsetsBatchDevice")
        flat_ran(h, ctx)
        g, gs, ge = out.cpu().numpy(), sts.cpu().numpy(), ens.cpu().numpy()
        assert (g[cap:] == -7).all() and (gs[cap:] == -7).all() and (ge[cap:] == -7).all(), ctx
        same(ctx, name, ido.cpu().numpy(), woff, [("ids", g[:cap], wids), ("first bytes", gs[:cap], ws), ("last bytes", ge[:cap], we)])
    finally:
        bf.free_model(h)
