"""GPU: IdsToBucketedRowsBatchDevice / IdsToBucketedRowsBatch (bf_kernels_bucket.hip) and the Python calls above them against the sequential
restatement of the specification (bucketed_cases.restate), by exact equality over canary-filled buffers: sequence counts around a wave, the sort's
tile and several blocks, one to three radix passes, the width patterns (all equal = the stability check), multiples, budgets, both caps, both
store paths, determinism, the BfReserve and status contracts, refused arguments, the host form, and text -> bucketed batches end to end against
the stored reference ids (tests/golden/rows/encode_ids.json)."""
import ctypes

import numpy as np
import pytest
import torch

import bfutil
import blingfire_amd as bf
import bucketed_cases as bc
import rows_cases as rc

pytestmark = pytest.mark.gpu

CANARY = 0x5A
E_ARG, E_CAPACITY = -1, -3
vp = ctypes.c_void_p
NAMES = ("rows", "mask", "order", "seq_pos", "first", "len", "cell", "counts")
DTYPES = (torch.int32, torch.uint8, torch.int32, torch.int32, torch.int32, torch.int32, torch.int64, torch.int64)


@pytest.fixture(scope="module", params=["wordpiece", "i2w"])
def h(request):
    hm = bf.load_model(bfutil.model_path(bfutil.bert_model_name() if request.param == "wordpiece" else "bert_base_tok.i2w"))
    yield hm
    bf.free_model(hm)


def status(hm):
    torch.cuda.synchronize()
    return bf.lib().BfLastStatus(vp(hm))


def device_call(hm, a, outs, cells_cap, batches_cap, **kw):
    a = dict(a, **kw)
    d_ids, d_off = (None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (a["ids"], a["off"]))
    p = [None if o is None else o.data_ptr() for o in outs]
    return bf.lib().IdsToBucketedRowsBatchDevice(vp(hm) if hm else None, None if d_ids is None else d_ids.data_ptr(), a["ids_len"], None if d_off is None else d_off.data_ptr(),
                                                 a["nseq"] if "nseq" in a else len(a["off"]) - 1, a["max_len"], a["cls"], a["sep"], a["pad"], a["multiple"], a["max_cells"], a["max_rows"],
                                                 a.get("flags", 0), p[0], p[1], cells_cap, p[2], p[3], p[4], p[5], p[6], batches_cap, p[7], None)


def check_device(hm, args, want, cells_cap=None, batches_cap=None, take=(True,) * 8, shift=0):
    """one call over canary-filled buffers, every taken output `shift` elements into its buffer: what the specification says is written equals the
    restatement, every byte around it is untouched, the status word is the restatement's; -> the buffers' bytes"""
    B, C = (int(x) for x in want["counts"])
    nseq = len(args["off"]) - 1
    cells_cap, batches_cap = C if cells_cap is None else cells_cap, B if batches_cap is None else batches_cap
    sizes = (cells_cap, cells_cap, nseq, nseq, batches_cap + 1, batches_cap + 1, batches_cap + 1, 2)
    valid = (min(C, cells_cap),) * 2 + (nseq, nseq) + (min(B, batches_cap) + 1,) * 3 + (2,)
    bufs = [torch.full(((n + 64) * t.itemsize,), CANARY, dtype=torch.uint8, device="cuda").view(t) for n, t in zip(sizes, DTYPES)]
    assert device_call(hm, args, [b[shift:] if t else None for b, t in zip(bufs, take)], cells_cap, batches_cap) == 0
    st = status(hm)
    got = [b.cpu().numpy() for b in bufs]
    for name, g, n, t in zip(NAMES, got, valid, take):
        n = n if t else 0
        assert np.array_equal(g[shift:shift + n], want[name][:n]), name
        assert (np.delete(g, np.s_[shift:shift + n]).view(np.uint8) == CANARY).all(), name
    assert st == (want["status"] | int((C > cells_cap and any(take[:2])) or (B > batches_cap and any(take[4:7]))))
    return got


# ---- sizes: every sequence count, the other axes rotating with it; 300,000 leaves the scan of the digit counts more than one block
@pytest.mark.parametrize("i,nseq", list(enumerate(bc.NSEQ + [300000])))
def test_sizes(h, i, nseq):
    max_len = 200 if nseq > 5000 else bc.MAX_LENS[i % 6]
    check_device(h, *bc.case(nseq, max_len, bc.PATTERNS[i % 4], bc.MULTIPLES[i % 3], 16384 if max_len < 65535 else "min"))


@pytest.mark.parametrize("max_len", bc.MAX_LENS)
@pytest.mark.parametrize("nseq", [65, 2049])
def test_passes(h, max_len, nseq):
    check_device(h, *bc.case(nseq, max_len, "random", 8, "min"))


@pytest.mark.parametrize("pattern", bc.PATTERNS)
@pytest.mark.parametrize("multiple", bc.MULTIPLES)
def test_patterns(h, pattern, multiple):
    args, want = bc.case(4097, 255, pattern, multiple, 4096)
    check_device(h, args, want)
    if pattern == "equal":
        assert np.array_equal(want["order"], np.arange(4097))              # ties keep their input order
    if pattern == "empty":
        assert (want["len"][:-1] == multiple).all() and not want["mask"].any()
    assert want["status"] == (8 if pattern == "bad" else 0)


@pytest.mark.parametrize("budget,max_rows", [("min", 0), ("one", 0), (4096, 1), (4096, 0), (4096, 7)])
def test_budgets(h, budget, max_rows):
    args, want = bc.case(1025, 24, "random", 8, budget, max_rows)                # lengths up to 23: some units reach max_len
    check_device(h, args, want)
    assert {("min", 0): want["first"][1] == 1, ("one", 0): want["counts"][0] == 1, (4096, 1): want["counts"][0] == 1025}.get((budget, max_rows), True)


@pytest.mark.parametrize("multiple", [8, 3])
def test_caps_and_store_paths(h, multiple):
    args, want = bc.case(513, 200, "random", multiple, 2048)
    B, C = (int(x) for x in want["counts"])
    assert B > 4
    for shift in (0, 1):                                   # 16-byte aligned outputs against odd natural alignments
        check_device(h, args, want, shift=shift)
        check_device(h, args, want, batches_cap=B - 3, shift=shift)
        check_device(h, args, want, cells_cap=int(want["cell"][2]) + int(want["len"][2]) + 5, shift=shift)      # ends inside a row
        check_device(h, args, want, cells_cap=0, batches_cap=0, shift=shift)
    check_device(h, args, want, take=(False, False) + (True,) * 6)           # the size query
    check_device(h, args, want, cells_cap=3, batches_cap=1, take=(False,) * 7 + (True,))      # nothing taken, nothing lost
    check_device(h, args, want, take=(True, False, False, False, True, False, False, True))


def test_determinism(h):
    args, want = bc.case(12293, 255, "random", 8, 16384)
    a, b = check_device(h, args, want), check_device(h, args, want)
    hm = bf.load_model(bfutil.model_path("bert_base_tok.i2w"))
    try:
        c = check_device(hm, args, want)
    finally:
        bf.free_model(hm)
    assert all(x.tobytes() == y.tobytes() == z.tobytes() for x, y, z in zip(a, b, c))


def test_reserve_and_status_contracts():
    args, want = bc.case(4097, 65535, "bad", 8, "min")
    clean = bc.case(65, 200, "random", 8, "min")
    hm = bf.load_model(bfutil.model_path("bert_base_tok.i2w"))
    try:
        assert bf.lib().BfReserve(vp(hm), 4097, 1 << 12, 0) == 0
        grows = bf.workspace_grows()
        check_device(hm, args, want)
        assert bf.workspace_grows() == grows, "the first call on the reserved handle allocated device memory"
        assert want["status"] == 8
        check_device(hm, *clean)                            # behind a call that set a status bit: its own status, 0
    finally:
        bf.free_model(hm)


def test_refused_arguments(h):
    args, want = bc.case(65, 200, "bad", 8, "min")
    counts = torch.zeros(2, dtype=torch.int64, device="cuda")
    outs = [None] * 7 + [counts]
    check_device(h, args, want)
    assert status(h) == 8                                   # the word every refusal below must leave alone
    for bad in (dict(max_len=0), dict(max_len=(1 << 20) + 1), dict(max_len=2), dict(multiple=0), dict(max_cells=199), dict(multiple=64, max_cells=255),
                dict(max_rows=-1), dict(flags=1), dict(nseq=-1), dict(nseq=1 << 31), dict(ids_len=-1), dict(off=None, nseq=65), dict(ids=None)):
        assert device_call(h, args, outs, 0, 0, **bad) == E_ARG, bad
    assert device_call(h, args, outs, -1, 0) == E_ARG and device_call(h, args, outs, 0, -1) == E_ARG
    assert device_call(h, args, [None] * 8, 0, 0) == E_ARG and device_call(None, args, outs, 0, 0) == E_ARG
    assert status(h) == 8
    assert device_call(h, args, outs, 0, 0, max_len=1, cls=-1, sep=-1, multiple=1, max_cells=1) == 0 and status(h) == 8 and counts.tolist() == [65, 65]


@pytest.mark.parametrize("nseq", [0, 65, 4097])
def test_host_form(h, nseq):
    args, want = bc.case(nseq, 256, "random", 8, 2048)
    got = bf.ids_to_bucketed_rows_batch(h, args["ids"], args["off"], 256, args["max_cells"], bc.CLS, bc.SEP, bc.PAD, 8)
    for name, g in zip(NAMES, got):
        assert g.dtype == want[name].dtype and np.array_equal(g, want[name]), name
    B, C = (int(x) for x in want["counts"])
    for cells_cap, batches_cap in ((C - 1, B), (C, B - 1)) if nseq else ():
        outs = [np.full(n, CANARY, dtype=w.dtype) for n, w in zip((C, C, nseq, nseq, B + 1, B + 1, B + 1, 2), (want[k] for k in NAMES))]
        r = bf.lib().IdsToBucketedRowsBatch(vp(h), args["ids"].ctypes.data, args["off"].ctypes.data, nseq, 256, bc.CLS, bc.SEP, bc.PAD, 8, args["max_cells"], 0, 0,
                                            outs[0].ctypes.data, outs[1].ctypes.data, cells_cap, outs[2].ctypes.data, outs[3].ctypes.data, outs[4].ctypes.data,
                                            outs[5].ctypes.data, outs[6].ctypes.data, batches_cap, outs[7].ctypes.data)
        assert r == E_CAPACITY
        assert all(np.array_equal(outs[k], want[NAMES[k]]) for k in (2, 3, 7)) and all((outs[k] == CANARY).all() for k in (0, 1, 4, 5, 6))


@pytest.mark.parametrize("model", sorted(rc.ENCODE_MODELS))
def test_text_to_bucketed_batches(model):
    sp, docs, max_len = rc.ENCODE_MODELS[model], rc.encode_docs(), 16
    ref_ids, ref_off = rc.fixture_ids(rc.load_fixture(), model, max_len - 2)       # the stored reference ids at max_len = body
    want = bc.restate(ref_ids, ref_off, max_len, sp["cls_id"], sp["sep_id"], sp["pad_id"], 4, 32)
    hm = bf.load_model(bfutil.model_path(model))
    try:
        d_text, d_off = (torch.from_numpy(x.copy()).cuda() for x in bf.pack_docs(docs))
        for caps in ({}, dict(cells_cap=int(want["counts"][1]), batches_cap=int(want["counts"][0]))):
            got = bf.encode_bucketed_batch_device(hm, d_text, d_off, max_len, sp["cls_id"], sp["sep_id"], sp["pad_id"], 32, 4, unk=sp["unk"], **caps)
            assert status(hm) == 0
            for name, g in zip(NAMES, got):
                assert np.array_equal(g.cpu().numpy(), want[name]), name
            views = list(bf.bucketed_views(got[0], got[1], *got[4:]))
            assert [tuple(r.shape) for r, _, _ in views] == [tuple(m.shape) for _, m, _ in views] == [
                (int(want["first"][b + 1] - want["first"][b]), int(want["len"][b])) for b in range(len(views))] and len(views) == want["counts"][0] > 1
            assert [s.start for _, _, s in views] == want["first"][:-1].tolist()
    finally:
        bf.free_model(hm)
