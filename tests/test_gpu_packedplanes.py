"""GPU: IdsToPackedRowsPlanesBatchDevice / IdsToPackedRowsPlanesBatch (k_packed_planes in bf_kernels_packed.hip) and the Python calls above them
against the restatement of the specification (packedplanes_cases.restate_packed_planes over packed_cases.restate): the parameter table with the
base outputs held byte for byte to the base call's, every subset of NULL planes and outputs over canary-filled buffers, unaligned planes, the
capacity guard, the scale edges, bad ranges and an overflowed tokenizer call in front, refused arguments, the host form, text -> packed rows
with offset planes end to end, whole-word MLM over packed rows, the reserve contract and the status word."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import bfutil
import blingfire_amd as bf
import mlm_cases as mc
import mlmcap_cases as cc
import packed_cases as pc
import packedplanes_cases as pp
import rows_cases as rc

pytestmark = pytest.mark.gpu

CANARY = pp.CANARY
E_ARG, E_CAPACITY = -1, -3
C, S, P = pc.CLS, pc.SEP, pc.PAD
ALL = (True,) * 6                  # rows, seg, pos, row_first_seq, seq_row, seq_col
NONE = (False,) * 6
vp, I32 = ctypes.c_void_p, ctypes.c_int32


@pytest.fixture(scope="module")
def h():
    hm = bf.load_model(bfutil.model_path(bfutil.bert_model_name()))
    yield hm
    bf.free_model(hm)


def status(hm):
    torch.cuda.synchronize()
    return bf.lib().BfLastStatus(vp(hm))


def ptr(t):
    return None if t is None else t.data_ptr()


def dev(x, dtype=np.int32):
    return torch.from_numpy(np.array(x, dtype=dtype, order="C")).cuda()


def canary(n):
    return torch.full((n,), CANARY, dtype=torch.int32, device="cuda")


def base_call(hm, d_ids, ids_len, d_off, nseq, L, cls, sep, outs, cap, nrows):
    return bf.lib().IdsToPackedRowsBatchDevice(vp(hm), ptr(d_ids), ids_len, ptr(d_off), nseq, L, cls, sep, P, 0, *[ptr(o) for o in outs[:4]], cap,
                                               *[ptr(o) for o in outs[4:]], ptr(nrows), None)


def planes_call(hm, d_ids, ids_len, d_off, nseq, L, cls, sep, outs, cap, nrows, srcs, fills, planes, nplanes=None, flags=0):
    """outs: the six base outputs (tensors or None); srcs / planes: tensors or None per plane, or None for a NULL array"""
    n = len(fills) if nplanes is None else nplanes
    arr = lambda xs: None if xs is None else (vp * max(len(xs), 1))(*[ptr(x) for x in xs])
    c_fill = None if fills is None else (I32 * max(len(fills), 1))(*fills)
    return bf.lib().IdsToPackedRowsPlanesBatchDevice(vp(hm), ptr(d_ids), ids_len, ptr(d_off), nseq, L, cls, sep, P, flags, *[ptr(o) for o in outs[:4]], cap,
                                                     *[ptr(o) for o in outs[4:]], ptr(nrows), n, arr(srcs), c_fill, arr(planes), None)


def check(hm, ids, off, L, cls, sep, nplanes=2, cap=None, ids_len=None, outs=ALL, take=None, want=None, against_base=False, d_src=None, src=None):
    """one planes call over canary-filled buffers of `cap` rows (default: R) with tail elements the call must not touch: every plane taken equals
    the restatement below min(cap, R) rows and nothing behind them changed; the base outputs are what packed_cases.restate says, and with
    against_base byte for byte what the base call writes into buffers of the same kind; the status word is the call's own"""
    n_ids = len(ids) if ids_len is None else ids_len
    if src is None:
        src = pp.sources(len(ids), nplanes, seed=L)
    fills = pp.FILLS[:nplanes]
    take = [True] * nplanes if take is None else list(take)
    if want is None:
        want = (pc.restate(ids, off, L, cls, sep, P, ids_len=n_ids), pp.restate_packed_planes(off, L, cls, sep, src, fills, ids_len=n_ids))
    base, wpl = want
    R, nseq, key = base[6], len(off) - 1, (L, cls, sep, cap, outs, take)
    cap = R if cap is None else cap
    d_ids, d_off = dev(ids), dev(off, np.int64)
    if d_src is None:
        d_src = [dev(s) for s in src]
    sizes = (cap * L, cap * L, cap * L, cap + 1, nseq, nseq)
    bufs = [canary(n + 64) for n in sizes]
    pbufs = [canary(cap * L + 64) for _ in range(nplanes)]
    nrows = torch.full((3,), -7, dtype=torch.int64, device="cuda")
    use = [b if u else None for b, u in zip(bufs, outs)]
    r = planes_call(hm, d_ids, n_ids, d_off, nseq, L, cls, sep, use, cap, nrows, d_src, fills, [b if t else None for b, t in zip(pbufs, take)])
    assert r == 0, key
    st = status(hm)
    assert nrows.cpu().tolist() == [R, -7, -7], key
    k = min(cap, R)
    valid = (k * L, k * L, k * L, k + 1, nseq, nseq)
    for i, (b, w) in enumerate(zip(bufs, base[:6])):
        g = b.cpu().numpy()
        n = valid[i] if outs[i] else 0
        assert np.array_equal(g[:n], w.reshape(-1)[:n]), (key, "base output", i)
        assert (g[n:] == CANARY).all(), (key, "base output", i)
    for i, (b, w, t) in enumerate(zip(pbufs, wpl, take)):
        g = b.cpu().numpy()
        n = k * L if t else 0
        assert np.array_equal(g[:n], w.reshape(-1)[:n]), (key, "plane", i)
        assert (g[n:] == CANARY).all(), (key, "plane", i)
    assert st == (base[7] | (1 if R > cap and (any(outs[:4]) or any(take)) else 0)), (key, st)
    if against_base:
        bbufs = [canary(n + 64) for n in sizes]
        nrows_b = torch.full((3,), -7, dtype=torch.int64, device="cuda")
        assert base_call(hm, d_ids, n_ids, d_off, nseq, L, cls, sep, [b if u else None for b, u in zip(bbufs, outs)], cap, nrows_b) == 0
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(bufs, bbufs)) and torch.equal(nrows, nrows_b), key
    return want


# ---- 1. the parameter table
@pytest.mark.parametrize("L", pc.TABLE_L)
def test_1_parameter_table(h, L):
    n = 0
    for l, cls, sep in pc.table():
        if l != L:
            continue
        ids, off = pc.synthetic(pc.geometry(L, cls, sep), seed=n)
        for nplanes in (1, 2, 4):
            check(h, ids, off, L, cls, sep, nplanes, against_base=True)
        n += 1
    assert n > 0


# ---- 2. subsets
def test_2_no_planes_is_the_base_call(h):
    ids, off = pc.mixed(40, 11, 8, C, S)
    want = pc.restate(ids, off, 8, C, S, P)
    for cap in (want[6], want[6] - 1):
        check(h, ids, off, 8, C, S, nplanes=0, cap=cap, want=(want, []), against_base=True)
        check(h, ids, off, 8, C, S, nplanes=0, cap=cap, outs=NONE, want=(want, []), against_base=True)          # the size query: no drop reported
    # the three arrays may be NULL then
    d_ids, d_off = dev(ids), dev(off, np.int64)
    nrows = torch.zeros(1, dtype=torch.int64, device="cuda")
    assert planes_call(h, d_ids, len(ids), d_off, len(off) - 1, 8, C, S, [None] * 6, 0, nrows, None, None, None, nplanes=0) == 0
    assert status(h) == 0 and int(nrows.item()) == want[6]


def test_2_every_subset_of_null_planes(h):
    ids, off = pc.mixed(40, 11, 8, C, S)
    src = pp.sources(len(ids), 3, seed=8)
    want = (pc.restate(ids, off, 8, C, S, P), pp.restate_packed_planes(off, 8, C, S, src, pp.FILLS[:3]))
    R = want[0][6]
    for take in itertools.product((False, True), repeat=3):
        for outs in (ALL, NONE, (True, False, False, False, False, True), (False, False, False, True, True, False)):
            check(h, ids, off, 8, C, S, nplanes=3, outs=outs, take=take, want=want, src=src)
            check(h, ids, off, 8, C, S, nplanes=3, cap=R - 1, outs=outs, take=take, want=want, src=src)


# ---- 3. alignment
@pytest.mark.parametrize("L", [8, 5])
@pytest.mark.parametrize("shifts", [(0, 0), (1, 0), (0, 2), (3, 3), (2, 1), (0, 3)])
def test_3_alignment(h, L, shifts):
    """each plane `shift` elements (4, 8, 12 bytes) behind a 16-byte boundary, mixed with aligned ones and all aligned: the wide form (L = 8, all
    aligned) and the narrow form give the same cells; the sources and the ids one element into larger buffers"""
    ids, off = pc.mixed(50, 17, L, C, S)
    src = pp.sources(len(ids), 2, seed=3)
    want = pp.restate_packed_planes(off, L, C, S, src, pp.FILLS[:2])
    R, nseq = want[0].shape[0], len(off) - 1
    ids_buf = torch.full((len(ids) + 9,), 777777, dtype=torch.int32, device="cuda"); ids_buf[1:1 + len(ids)] = dev(ids)
    src_bufs = [torch.full((len(ids) + 9,), 555555, dtype=torch.int32, device="cuda") for _ in src]
    for b, s in zip(src_bufs, src):
        b[1:1 + len(ids)] = dev(s)
    bufs = [canary(R * L + 64) for _ in range(2)]
    assert all(b.data_ptr() % 16 == 0 for b in bufs)
    planes = [b[s:] for b, s in zip(bufs, shifts)]
    nrows = torch.zeros(1, dtype=torch.int64, device="cuda")
    assert planes_call(h, ids_buf[1:], len(ids), dev(off, np.int64), nseq, L, C, S, [None] * 6, R, nrows, [b[1:] for b in src_bufs], pp.FILLS[:2], planes) == 0
    assert status(h) == 0 and int(nrows.item()) == R
    for b, s, w in zip(bufs, shifts, want):
        g = b.cpu().numpy()
        assert np.array_equal(g[s:s + R * L], w.reshape(-1)) and (g[:s] == CANARY).all() and (g[s + R * L:] == CANARY).all(), (L, shifts)


# ---- 4. capacity
@pytest.mark.parametrize("L,cls,sep", [(8, C, S), (5, C, -1), (64, C, S)])
def test_4_capacity(h, L, cls, sep):
    ids, off = pc.mixed(90, 5 + L, L, cls, sep)
    src = pp.sources(len(ids), 2, seed=4)
    want = (pc.restate(ids, off, L, cls, sep, P), pp.restate_packed_planes(off, L, cls, sep, src, pp.FILLS[:2]))
    R = want[0][6]
    assert R > 4
    for cap in (0, 1, R - 1, R, R + 1):
        check(h, ids, off, L, cls, sep, cap=cap, want=want, src=src)                       # status bit 0 exactly when R > cap
        check(h, ids, off, L, cls, sep, cap=cap, outs=NONE, want=want, src=src)            # planes alone: the drop is still reported
        check(h, ids, off, L, cls, sep, cap=cap, outs=NONE, take=[False, False], want=want, src=src)      # nothing taken: nothing dropped


# ---- 5. scale edges
@pytest.mark.parametrize("nseq", [1, 2, 3, 4, 5, 63, 64, 65, 1023, 1024, 1025, 5000])
def test_5_sequence_counts_around_the_scan_tile(h, nseq):
    ids, off = pc.ragged([4] * nseq)                      # every unit fills a row: R = nseq
    check(h, ids, off, 4, -1, -1, nplanes=1)
    ids, off = pc.mixed(nseq, nseq, 12, C, S)
    check(h, ids, off, 12, C, S)
    ids, off = pc.mixed(nseq, nseq + 1, 7, -1, S)
    check(h, ids, off, 7, -1, S)


def test_5_empty_sequences_inside_one_row(h):
    ids, off = pc.ragged([3] + [0] * 100000 + [2])
    base, planes = check(h, ids, off, 8, -1, -1, nplanes=1)
    src = pp.sources(len(ids), 1, seed=8)[0]
    assert base[6] == 1 and planes[0][0].tolist() == src.tolist() + [pp.FILLS[0]] * 3


def test_5_one_sequence_of_three_bodies(h):
    for L, cls, sep in ((8, C, S), (64, -1, -1), (5, -1, S)):
        body = pc.geometry(L, cls, sep)
        ids, off = pc.ragged([2, 3 * body, 1])
        base, planes = check(h, ids, off, L, cls, sep)
        src = pp.sources(len(ids), 2, seed=L)
        r, c = base[4][1], base[5][1] + (1 if cls >= 0 else 0)
        assert planes[1][r][c:c + body].tolist() == src[1][2:2 + body].tolist()              # the first `body` elements, none behind them


def test_5_more_lanes_than_one_pass_of_the_grid(h):
    """one unit per row at L = 9 (the narrow form: a lane per cell) whose cells outnumber the lanes of the largest grid, 8 blocks of 256 per
    compute unit: the grid-stride step of k_packed_planes runs"""
    L = 9
    lanes = torch.cuda.get_device_properties(0).multi_processor_count * 8 * 256
    nseq = lanes // L + 8000
    assert nseq * L > lanes
    rnd = np.random.RandomState(9)
    ids, off = pc.ragged(rnd.randint(5, 12, size=nseq).tolist(), 1000)                      # two units never share a row: R = nseq
    base, _ = check(h, ids, off, L, -1, -1, outs=NONE)
    assert base[6] == nseq


# ---- 6. bad ranges, an overflowed tokenizer call in front
def end_of_allocation(values):
    """`values` in the last elements of a tensor of 16 MiB, a size the caching allocator serves with an allocation of its own: the array ends where
    the allocation ends"""
    buf = torch.zeros(1 << 22, dtype=torch.int32, device="cuda")
    if len(values):
        buf[-len(values):] = dev(values)
    return buf, buf[len(buf) - len(values):]


def test_6_bad_ranges(h):
    ids = (1000 + np.arange(60)).astype(np.int32)
    for off, ids_len in pp.bad_range_cases():
        src = pp.sources(ids_len, 2, seed=6)
        keep, d_src = zip(*[end_of_allocation(s) for s in src])
        assert all(t.numel() == ids_len for t in d_src)
        base, planes = check(h, ids, off, 8, C, S, ids_len=ids_len, src=src, d_src=list(d_src))
        assert base[7] == 8
        for q in range(len(off) - 1):
            if off[q] < 0 or off[q + 1] < off[q] or off[q + 1] > ids_len:                   # read as empty: no id cells
                r, c = base[4][q], base[5][q]
                assert (planes[0][r][c:c + 2] == pp.FILLS[0]).all() and base[0][r][c:c + 2].tolist() == [C, S]
        del keep


def test_6_behind_a_tokenizer_call_that_overflowed(h):
    """TextToIdsWithOffsetsBatchDevice with an ids_cap too small, the planes call behind it on the same stream with ids_len = that capacity and
    no synchronisation between them; ids, starts and ends each end where their allocation ends"""
    docs = [b"hello world again", b"unaffable telescope", b"a b c d e f g h i j k l m n o p", b"the end"]
    text, doff = bf.pack_docs(docs)
    full_ids, full_st, full_en, full_off = bf.text_to_ids_with_offsets_batch(h, (text, doff), 64, 100)
    cap = int(full_off[2]) + 3                                 # documents 0 and 1 fit, 2 and 3 do not
    d_text, d_doff = dev(text, np.uint8), dev(doff, np.int64)
    keep, (d_ids, d_st, d_en) = zip(*[end_of_allocation(np.full(cap, -1, dtype=np.int32)) for _ in range(3)])
    d_idoff = torch.empty(len(docs) + 1, dtype=torch.int64, device="cuda")
    r = bf.lib().TextToIdsWithOffsetsBatchDevice(vp(h), ptr(d_text), ptr(d_doff), len(docs), d_text.numel(), ptr(d_ids), ptr(d_st), ptr(d_en), cap, ptr(d_idoff), 64, 100, None)
    assert r == 0
    got = bf.ids_to_packed_rows_batch_device(h, d_ids, d_idoff, 16, C, S, P, rows_cap=4, planes=[d_st, d_en], fill=[-1, -1])
    assert status(h) == 8 and len(got) == 9
    want = pc.restate(full_ids, full_off, 16, C, S, P, ids_len=cap)
    wpl = pp.restate_packed_planes(full_off, 16, C, S, [full_st[:cap], full_en[:cap]], [-1, -1], ids_len=cap)
    R = want[6]
    assert R <= 4 and int(got[6].item()) == R
    for g, w in zip(got[:3] + got[7:], list(want[:3]) + wpl):
        assert np.array_equal(g.cpu().numpy()[:R], w)
    c = want[5][2]
    assert (wpl[0][want[4][2]][c:c + 2] == -1).all() and wpl[0][0][1] == full_st[0] and wpl[1][0][1] == full_en[0]
    del keep


# ---- 7. arguments
def test_7_refused_arguments(h):
    ids = torch.arange(4, dtype=torch.int32, device="cuda"); off = torch.tensor([0, 4], dtype=torch.int64, device="cuda")
    src = [torch.arange(4, dtype=torch.int32, device="cuda") for _ in range(4)]
    out = [canary(8) for _ in range(5)]
    nrows = torch.full((1,), -1, dtype=torch.int64, device="cuda")

    def call(hm=h, d_ids=ids, ids_len=4, nseq=1, cap=1, d_off=off, d_nrows=nrows, L=8, cls=1, sep=2, flags=0, n=2, srcs=src[:2], fills=(-1, -1), planes=out[:2]):
        return planes_call(hm, d_ids, ids_len, d_off, nseq, L, cls, sep, [None] * 6, cap, d_nrows, srcs, fills, planes, nplanes=n, flags=flags)
    assert call() == 0 and status(h) == 0 and nrows.item() == 1
    assert out[0].cpu().tolist() == [-1, 0, 1, 2, 3, -1, -1, -1]
    # a status word to be left alone: one row dropped from a taken plane
    assert call(cap=0) == 0 and status(h) == 1
    for bad in (dict(n=-1), dict(n=5, srcs=src + src[:1], fills=(0,) * 5, planes=out), dict(fills=None), dict(planes=None), dict(srcs=None), dict(srcs=[src[0], None]),
                dict(L=0), dict(L=2), dict(L=(1 << 20) + 1), dict(flags=1), dict(hm=None), dict(nseq=-1), dict(nseq=1 << 31), dict(cap=-1), dict(d_off=None),
                dict(d_nrows=None), dict(d_ids=None), dict(ids_len=-1)):
        assert call(**bad) == E_ARG, bad
        assert bf.lib().BfLastStatus(vp(h)) == 1, bad                              # a refused call does not touch the status word
    assert call(n=4, srcs=src, fills=(0,) * 4, planes=out[:4]) == 0 and status(h) == 0
    assert call(planes=[None, out[1]]) == 0 and call(planes=[None, None], cap=0) == 0 and status(h) == 0      # NULL planes are skipped; none taken: nothing dropped
    assert call(d_ids=None, ids_len=0, srcs=None) == 0 and status(h) == 8          # nothing to read: no sources needed; the sequence is outside [0, 0]
    assert call(d_ids=None, ids_len=0, srcs=[None, None]) == 0 and status(h) == 8
    # the host form
    hi = np.arange(4, dtype=np.int32); ho = np.array([0, 4], dtype=np.int64)
    hs = [np.arange(4, dtype=np.int32) for _ in range(2)]; hp = [np.full(8, CANARY, dtype=np.int32) for _ in range(2)]
    f = bf.lib().IdsToPackedRowsPlanesBatch
    arr = lambda xs: (vp * 2)(*[None if x is None else x.ctypes.data for x in xs])
    fills = (I32 * 2)(-1, -1)
    pre = (vp(h), hi.ctypes.data, ho.ctypes.data, 1, 8, 1, 2, 0, 0, None, None, None, None, 1, None, None)
    assert f(*pre, 2, arr(hs), fills, arr(hp)) == 1 and hp[1].tolist() == [-1, 0, 1, 2, 3, -1, -1, -1]
    assert f(*pre, 5, arr(hs), fills, arr(hp)) == E_ARG and f(*pre, -1, arr(hs), fills, arr(hp)) == E_ARG
    assert f(*pre, 2, None, fills, arr(hp)) == E_ARG and f(*pre, 2, arr([hs[0], None]), fills, arr(hp)) == E_ARG
    assert f(*pre, 2, arr(hs), None, arr(hp)) == E_ARG and f(*pre, 2, arr(hs), fills, None) == E_ARG
    assert f(None, *pre[1:], 2, arr(hs), fills, arr(hp)) == E_ARG
    assert f(*pre, 0, None, None, None) == 1


def test_7_no_sequences(h):
    want = (pc.restate([], [0], 8, C, S, P), [np.zeros((0, 8), dtype=np.int32)] * 2)
    check(h, np.zeros(0, dtype=np.int32), np.zeros(1, dtype=np.int64), 8, C, S, cap=4, want=want, src=[np.zeros(0, dtype=np.int32)] * 2)
    got = bf.ids_to_packed_rows_planes_batch(h, np.zeros(0, dtype=np.int32), np.zeros(1, dtype=np.int64), 8, C, S, src=[np.zeros(0, dtype=np.int32)], fill=[-1])
    assert [g.shape for g in got[:6]] == [(0, 8)] * 3 + [(1,), (0,), (0,)] and [g.shape for g in got[6]] == [(0, 8)]


def test_7_handles_of_every_kind():
    import w2h_cases
    ids, off = pc.synthetic(6)
    kinds = []
    for path in (bfutil.model_path(bfutil.bert_model_name()), bfutil.model_path("gpt2.bin"), bfutil.model_path("bert_base_tok.i2w"), w2h_cases.FIXTURE):
        hm = bf.load_model(path)
        try:
            kinds.append(bf.lib().BfModelKind(vp(hm)))
            assert bf.lib().BfReserve(vp(hm), 64, 1 << 12, 0) == 0
            check(hm, ids, off, 8, C, S)
        finally:
            bf.free_model(hm)
    assert kinds == [0, 3, 5, 6]                               # WordPiece, BPE, [i2w] only, [w2h] only


# ---- 8. the host form
def test_8_host_form(h):
    L = 8
    ids, off = pc.mixed(70, 23, L, C, S)
    ids = np.ascontiguousarray(ids, dtype=np.int32); off = np.ascontiguousarray(off, dtype=np.int64)
    src = pp.sources(len(ids), 2, seed=23)
    fills = pp.FILLS[:2]
    want, wpl = check(h, ids, off, L, C, S, src=src)           # the device form equals the restatement ...
    R, nseq = want[6], len(off) - 1
    got = bf.ids_to_packed_rows_planes_batch(h, ids, off, L, C, S, P, src=src, fill=fills)
    for g, w in zip(list(got[:6]) + got[6], list(want[:6]) + wpl):      # ... and so does the host form
        assert g.dtype == np.int32 and g.shape == w.shape and np.array_equal(g, w)
    f = bf.lib().IdsToPackedRowsPlanesBatch
    pre = (vp(h), ids.ctypes.data, off.ctypes.data, nseq, L, C, S, P, 0)
    c_src = (vp * 2)(*[s.ctypes.data for s in src]); c_fill = (I32 * 2)(*fills)
    arr = lambda xs: (vp * 2)(*[None if x is None else x.ctypes.data for x in xs])
    # the size query: the four row outputs and every plane NULL, whatever rows_cap is
    seq = [np.full(nseq, CANARY, dtype=np.int32) for _ in range(2)]
    assert f(*pre, None, None, None, None, 0, seq[0].ctypes.data, seq[1].ctypes.data, 2, c_src, c_fill, arr([None, None])) == R
    assert np.array_equal(seq[0], want[4]) and np.array_equal(seq[1], want[5])
    # BF_E_CAPACITY: the sequence outputs complete, nothing else written -- with the row outputs, and with a plane alone
    for cap in (0, R - 1):
        for with_rows in (True, False):
            base = [np.full((cap, L), CANARY, dtype=np.int32) for _ in range(3)] + [np.full(cap + 1, CANARY, dtype=np.int32)]
            planes = [np.full((cap + 1, L), CANARY, dtype=np.int32) for _ in range(2)]      # (a row more than the capacity: an array with an address)
            seq = [np.full(nseq, CANARY, dtype=np.int32) for _ in range(2)]
            r = f(*pre, *[b.ctypes.data if with_rows else None for b in base], cap, seq[0].ctypes.data, seq[1].ctypes.data, 2, c_src, c_fill, arr([None, planes[1]]))
            assert r == E_CAPACITY, (cap, with_rows)
            assert all((b == CANARY).all() for b in base + planes)
            assert np.array_equal(seq[0], want[4]) and np.array_equal(seq[1], want[5])
    # one plane alone in a buffer larger than needed
    planes = [np.full((R + 2, L), CANARY, dtype=np.int32) for _ in range(2)]
    assert f(*pre, None, None, None, None, R + 2, None, None, 2, c_src, c_fill, arr([planes[0], None])) == R
    assert np.array_equal(planes[0][:R], wpl[0]) and (planes[0][R:] == CANARY).all() and (planes[1] == CANARY).all()
    # sources staged from id_offsets[0] on: offsets that do not begin at 0
    off2 = off[5:].copy()
    want2 = pp.restate_packed_planes(off2, L, C, S, src, fills)
    got2 = bf.ids_to_packed_rows_planes_batch(h, ids, off2, L, C, S, P, src=src, fill=fills)
    assert all(np.array_equal(g, w) for g, w in zip(got2[6], want2))


# ---- 9. end to end
@pytest.fixture(scope="module")
def fx():
    return rc.load_fixture()


@pytest.mark.parametrize("model", sorted(rc.ENCODE_MODELS))
@pytest.mark.parametrize("L", [16, 8])
def test_9_text_to_packed_rows_with_offsets(fx, model, L):
    sp = rc.ENCODE_MODELS[model]
    docs = rc.encode_docs()
    ref_ids, ref_off = rc.fixture_ids(fx, model, L - 2)       # the stored reference ids at max_len = body
    want = pc.restate(ref_ids, ref_off, L, sp["cls_id"], sp["sep_id"], sp["pad_id"])
    R = want[6]
    hm = bf.load_model(bfutil.model_path(model))
    try:
        text, off = bf.pack_docs(docs)
        _, st, en, id_off = bf.text_to_ids_with_offsets_batch(hm, (text, off), L - 2, sp["unk"])
        assert np.array_equal(id_off, ref_off)
        wpl = pp.restate_packed_planes(id_off, L, sp["cls_id"], sp["sep_id"], [st, en], [-1, -1])
        got = bf.encode_packed_batch_device(hm, dev(text, np.uint8), dev(off, np.int64), L, sp["cls_id"], sp["sep_id"], sp["pad_id"], sp["unk"], return_offsets=True)
        torch.cuda.synchronize()
        assert len(got) == 9 and int(got[6].item()) == R and [tuple(t.shape) for t in got[7:]] == [(R, L)] * 2
        for g, w in zip(got[:6] + got[7:], list(want[:6]) + wpl):
            assert g.dtype == torch.int32 and np.array_equal(g.cpu().numpy(), w)
        assert bf.lib().BfLastStatus(vp(hm)) == 0
        assert (got[7].cpu().numpy() >= 0).any() and not (got[7].cpu().numpy()[want[1] == 0] != -1).any()
    finally:
        bf.free_model(hm)


# ---- 10. whole-word MLM over packed rows
SPECIALS = [mc.CLS, mc.SEP, mc.PAD]
SENTENCES = ["The tokenization of unaffable embeddings is straightforward.", "Hello, world! This is a test.", "playing replayed unplayable players",
             "supercalifragilisticexpialidocious", "a", "", "internationalization and localization", "pretraining pretrained pretrains",
             "unbelievably unmistakable unforgettable", "rereading misreading proofreading", "antidisestablishmentarianism!", "one two three four five",
             "Whole-word masking keeps the pieces of a word together, whatever the tokenizer made of it.", "hyphen-ated words-and-more"]


@pytest.fixture(scope="module")
def corpus():
    text, off = bf.pack_docs([s.encode() for s in SENTENCES * 3])
    return dev(text, np.uint8), dev(off, np.int64)


@pytest.mark.parametrize("epoch", [0, 1])
def test_10_whole_word_mlm_over_packed_rows(h, corpus, epoch):
    L = 48
    base = bf.encode_packed_batch_device(h, *corpus, L, mc.CLS, mc.SEP, mc.PAD, return_offsets=True)      # the unmasked rows of the same call
    out = bf.encode_packed_mlm_batch_device(h, *corpus, L, mc.CLS, mc.SEP, mc.PAD, mc.MASK, mc.RAND_RANGE, seed=31, epoch=epoch, select_prob=0.5)
    torch.cuda.synchronize()
    n = int(base[6].item())
    assert len(out) == 10 and 1 < n < len(SENTENCES) * 3 and all(torch.equal(a, b) for a, b in zip(out[1:9], base[1:9]))
    rows, seg, st, en = (base[i].cpu().numpy() for i in (0, 1, 7, 8))
    kw = dict(special_ids=SPECIALS, probs=(0.5, 0.8, 0.1), seed=31, epoch=epoch)
    want = mc.restate_mlm(rows, None, seg, st, en, **kw)
    assert np.array_equal(out[0].cpu().numpy(), want[0]) and np.array_equal(out[9].cpu().numpy(), want[1])
    lab = want[1] != -100
    runs = mc.unit_runs(mc.heads(mc.eligible(rows, None, seg, SPECIALS), st, en))
    assert sum(len(x) for x in runs) > 20
    assert all(len(set(seg[r, a:z + 1].tolist())) == 1 for r, rr in enumerate(runs) for a, z in rr)            # no unit spans two sequences
    assert all(lab[r, a:z + 1].all() or not lab[r, a:z + 1].any() for r, rr in enumerate(runs) for a, z in rr)  # a unit is labelled whole, or not at all
    assert any(lab[r, a:z + 1].all() for r, rr in enumerate(runs) for a, z in rr)                                # and at least one unit of several cells is
    assert not lab[seg == 0].any() and not lab[np.isin(rows, SPECIALS)].any()
    # the capped form
    cap = bf.encode_packed_mlm_batch_device(h, *corpus, L, mc.CLS, mc.SEP, mc.PAD, mc.MASK, mc.RAND_RANGE, seed=31, epoch=epoch, select_prob=0.5, max_predictions=5)
    torch.cuda.synchronize()
    wcap = cc.restate_cap(rows, None, seg, st, en, max_pred=5, **kw)
    assert len(cap) == 13
    for g, w in zip((cap[0], cap[9], cap[10], cap[11], cap[12]), wcap):
        assert np.array_equal(g.cpu().numpy(), w)
    assert not np.array_equal(wcap[1], want[1])                # the cap binds somewhere


def test_10_whole_words_need_a_special_between_sequences(h, corpus):
    with pytest.raises(ValueError):
        bf.encode_packed_mlm_batch_device(h, *corpus, 48, None, None, mc.PAD, mc.MASK, mc.RAND_RANGE, seed=1)
    out = bf.encode_packed_mlm_batch_device(h, *corpus, 48, None, None, mc.PAD, mc.MASK, mc.RAND_RANGE, seed=1, whole_word=False)      # token by token is fine
    out2 = bf.encode_packed_mlm_batch_device(h, *corpus, 48, None, mc.SEP, mc.PAD, mc.MASK, mc.RAND_RANGE, seed=1)                       # one special is enough
    torch.cuda.synchronize()
    assert len(out) == 10 and len(out2) == 10


# ---- 11. the reserve contract
def test_11_reserved_calls_allocate_nothing():
    docs = rc.encode_docs() * 8
    text, off = bf.pack_docs(docs)
    sp = rc.ENCODE_MODELS["bert_base_tok.bin"]
    hm = bf.load_model(bfutil.model_path("bert_base_tok.bin"))
    try:
        bf.reserve(hm, len(docs), len(text), True)
        grows0 = bf.workspace_grows()
        d_text, d_off = dev(text, np.uint8), dev(off, np.int64)
        args = (hm, d_text, d_off, 16, sp["cls_id"], sp["sep_id"], sp["pad_id"], sp["unk"])
        a = bf.encode_packed_batch_device(*args, rows_cap=len(docs), return_offsets=True)
        torch.cuda.synchronize()
        assert bf.workspace_grows() == grows0, "the FIRST call on the reserved handle made the library allocate device memory (BfWorkspaceGrows)"
        R = int(a[6].item())
        assert 0 < R < len(docs) and len(a) == 9
        a = [t.cpu().numpy() for t in a]
        free0 = torch.cuda.mem_get_info()[0]
        b = bf.encode_packed_batch_device(*args, rows_cap=len(docs), return_offsets=True)
        torch.cuda.synchronize()
        free1 = torch.cuda.mem_get_info()[0]
        assert free1 == free0, "the device's free memory moved by %d bytes across a reserved call" % (free0 - free1)
        assert bf.workspace_grows() == grows0, "the repeated call made the library allocate device memory (BfWorkspaceGrows)"
        for i, (x, y) in enumerate(zip(a, b)):
            n = R + 1 if i == 3 else len(x) if i in (4, 5, 6) else R
            assert np.array_equal(x[:n], y.cpu().numpy()[:n]), i
        assert (a[7][:R] >= 0).any()
    finally:
        bf.free_model(hm)


# ---- 12. the status word is the call's own
def test_12_status_hygiene(h):
    ids, off = pc.mixed(30, 12, 8, C, S)
    bad_ids, bad = (1000 + np.arange(60)).astype(np.int32), np.array([0, 5, 3, 12, 20], dtype=np.int64)
    want = check(h, bad_ids, bad, 8, C, S)                     # sets bit 3
    assert want[0][7] == 8
    check(h, ids, off, 8, C, S)                                # the next call reports its own status: 0 (asserted inside)
    R = pc.restate(ids, off, 8, C, S, P)[6]
    check(h, ids, off, 8, C, S, cap=R - 1, outs=NONE)          # sets bit 0, from a plane alone
    check(h, ids, off, 8, C, S, outs=NONE)                     # 0 again
    check(h, bad_ids, bad, 8, C, S, cap=1)                     # both bits at once
