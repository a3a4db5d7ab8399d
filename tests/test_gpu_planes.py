"""GPU: the companion planes of the row stage (IdsToRowsPlanesBatch* / IdsToPairRowsPlanesBatch*, k_rowstage_planes), the span cells
(RowsSpanCellsBatchDevice, k_rows_span) and the Python calls above them against the restatements of plane_cases: both parameter tables with 1, 2
and 4 planes and every base output held to the base call, the capacity guard over canary-filled buffers, shifted plane bases, batch sizes
around the scan tile, very many windows and the grid-stride step, hostile inputs, the span cells at every group size, and text -> tensors with
offsets and answer cells end to end."""
import ctypes

import numpy as np
import pytest
import torch

import bfutil
import blingfire_amd as bf
import pair_cases as pc
import plane_cases as pl
import rows_cases as rc

pytestmark = pytest.mark.gpu

CANARY32, CANARY8 = pl.CANARY32, 0xA5
E_ARG, E_CAPACITY = -1, -3
vp, c_i32 = ctypes.c_void_p, ctypes.c_int32
FILLS = pl.FILLS
I32, U8 = torch.int32, torch.uint8
# per kind: the base call, the planes call, (dtype, per cell or per row) of every base output
KINDS = {"rows": ("IdsToRowsBatchDevice", "IdsToRowsPlanesBatchDevice", ((I32, True), (U8, True), (I32, False), (I32, False))),
         "pairs": ("IdsToPairRowsBatchDevice", "IdsToPairRowsPlanesBatchDevice", ((I32, True), (U8, True), (U8, True), (I32, False), (I32, False)))}


@pytest.fixture(scope="module")
def h():
    hm = bf.load_model(bfutil.model_path(bfutil.bert_model_name()))
    yield hm
    bf.free_model(hm)


def status(hm):
    torch.cuda.synchronize()
    return bf.lib().BfLastStatus(vp(hm))


def ptr(t):
    return None if t is None else t if isinstance(t, int) else t.data_ptr()


def dev(x, dtype=np.int32):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x, dtype=dtype)).cuda()


def ptr_array(items, n):
    return (vp * max(n, 1))(*[ptr(x) for x in items])


def rows_pre(hm, d_ids, ids_len, d_off, nseq, par, pad_id=rc.PAD):
    L, cls_id, sep_id, stride, max_rows, pad_left = par
    return (vp(hm), ptr(d_ids), ids_len, ptr(d_off), nseq, L, cls_id, sep_id, pad_id, stride, max_rows, 1 if pad_left else 0)


def pairs_pre(hm, d, len_a, len_b, nseq, par, pad_id=pc.PAD):
    L, cls_id, sep_id, double_sep, mode, max_a, stride, max_rows, pad_left = par
    return (vp(hm), ptr(d[0]), len_a, ptr(d[1]), ptr(d[2]), len_b, ptr(d[3]), nseq, L, cls_id, sep_id, pad_id, mode, max_a, stride, max_rows, pc.flags(pad_left, double_sep))


def call(kind, pre, L, cap, nseq, take=None, planes=None):
    """one device call over canary-filled buffers of cap rows (+ 64 elements that must not change either).  planes = (sides, fill, ptake): the
    planes call -- sides = one list of tensors / None per side (or None for a NULL array), ptake[k] False = a NULL entry of d_planes_out.
    -> (rc, base outputs, row offsets, planes, status) as numpy"""
    base_name, planes_name, outs = KINDS[kind]
    take = [True] * len(outs) if take is None else take
    bufs = [torch.full((cap * (L if cell else 1) + 64,), CANARY32 if dt == I32 else CANARY8, dtype=dt, device="cuda") for dt, cell in outs]
    r_off = torch.full((nseq + 1,), -1, dtype=torch.int64, device="cuda")
    args = [*pre, *[ptr(b) if t else None for b, t in zip(bufs, take)], cap, ptr(r_off)]
    pb = []
    if planes is not None:
        sides, fill, ptake = planes
        n = len(fill)
        pb = [torch.full((cap * L + 64,), CANARY32, dtype=I32, device="cuda") for _ in range(n)]
        args += [n, *[None if side is None else ptr_array(side, n) for side in sides], (c_i32 * max(n, 1))(*fill),
                 ptr_array([b if t else None for b, t in zip(pb, ptake)], n)]
    r = getattr(bf.lib(), planes_name if planes is not None else base_name)(*args, None)
    st = status(pre[0].value)
    return r, [b.cpu().numpy() for b in bufs], r_off.cpu().numpy(), [b.cpu().numpy() for b in pb], st


def check(kind, pre, L, nseq, want, sides, fill, cap=None, take=None, ptake=None, base=None):
    """the planes call against the restatement `want` = (planes, row_seq, row_first, row_offsets, status) and against the base call with the
    same arguments (returned, to be handed in again): base outputs byte for byte, planes exact below min(cap, total), canaries elsewhere"""
    total = len(want[1])
    cap = total if cap is None else cap
    n = len(fill)
    ptake = [True] * n if ptake is None else ptake
    ntake = len(KINDS[kind][2])
    take = [True] * ntake if take is None else take
    got = call(kind, pre, L, cap, nseq, take, (sides, fill, ptake))
    assert got[0] == 0, got[0]
    if base is None:
        base = call(kind, pre, L, cap, nseq, take)
        assert base[0] == 0 and np.array_equal(base[2], want[3])
        k = min(cap, total)
        for i, w in ((ntake - 2, want[1]), (ntake - 1, want[2])):          # (the base call itself: item and first id of every row)
            assert not take[i] or np.array_equal(base[1][i][:k], w[:k])
    for g, b in zip(got[1], base[1]):
        assert np.array_equal(g, b)
    assert np.array_equal(got[2], want[3])
    k = min(cap, total)
    for i in range(n):
        g = got[3][i]
        if ptake[i]:
            assert np.array_equal(g[:k * L], want[0][i][:k].reshape(-1)), ("plane", i, cap)
            assert (g[k * L:] == CANARY32).all(), ("past the capacity of plane", i, cap)
        else:
            assert (g == CANARY32).all(), ("a plane that was not taken", i)
    dropped = 1 if total > cap and (any(take) or any(ptake)) else 0
    assert got[4] == want[4] | dropped, (got[4], want[4], dropped)
    return base


def split(par):
    """the keyword arguments of the restatements for a table entry of either kind"""
    if len(par) == 6:
        return dict(zip(("L", "cls_id", "sep_id", "stride", "max_rows", "pad_left"), par))
    return dict(zip(("L", "cls_id", "sep_id", "double_sep", "mode", "max_a", "stride", "max_rows", "pad_left"), par))


def rows_case(hm, ids, off, par, src, fill, ids_len=None, **kw):
    """rows form: restatement, upload, check with every plane of `src`"""
    want = pl.restate_planes(off, src=src if ids_len is None else [s[:ids_len] for s in src], fill=fill, ids_len=ids_len, **split(par))
    d_ids, d_off, d_src = dev(ids), dev(off, np.int64), [dev(s) for s in src]
    pre = rows_pre(hm, d_ids, len(ids) if ids_len is None else ids_len, d_off, len(off) - 1, par)
    check("rows", pre, par[0], len(off) - 1, want, [d_src], fill, **kw)
    return want


# ---- 1. the parameter tables, nplanes 1, 2 and 4
@pytest.mark.parametrize("L", rc.TABLE_L)
def test_1_rows_table(h, L):
    n = 0
    for par in rc.table():
        if par[0] != L:
            continue
        ids, off = rc.synthetic(*rc.geometry(L, par[1], par[2], par[3]), seed=n)
        src = pl.sources(len(ids), 4, n, FILLS)                          # negative values, and values equal to the fill
        want = pl.restate_planes(off, src=src, fill=FILLS, **split(par))
        d_ids, d_off, d_src = dev(ids), dev(off, np.int64), [dev(s) for s in src]
        pre = rows_pre(h, d_ids, len(ids), d_off, len(off) - 1, par)
        base = None
        for k in (1, 2, 4):
            base = check("rows", pre, L, len(off) - 1, (want[0][:k],) + want[1:], [d_src[:k]], FILLS[:k], base=base)
        if n % 4 == 0:                                                   # the host form and the Python call above it
            k = (1, 2, 4)[(n // 4) % 3]
            _, cls_id, sep_id, stride, max_rows, pad_left = par
            got = bf.ids_to_rows_planes_batch(h, ids, off, L, cls_id, sep_id, rc.PAD, stride, max_rows, pad_left, src=src[:k], fill=FILLS[:k])
            plain = bf.ids_to_rows_batch(h, ids, off, L, cls_id, sep_id, rc.PAD, stride, max_rows, pad_left)
            assert len(got) == 6 and len(got[5]) == k and all(np.array_equal(a, b) for a, b in zip(got[:5], plain))
            assert all(g.dtype == np.int32 and np.array_equal(g, w) for g, w in zip(got[5], want[0]))
        n += 1
    assert n > 0


def pair_sides(n, d_a, d_b):
    """the side arrays a pairs entry runs with, by its number: both, A only, B only, neither (as NULL arrays), NULL entries mixed"""
    return [(1, [d_a[:1], d_b[:1]]), (2, [d_a[:2], None]), (2, [None, d_b[:2]]), (1, [None, None]),
            (4, [[d_a[0], None, d_a[2], None], [d_b[0], d_b[1], None, None]])]


@pytest.mark.parametrize("L", pc.TABLE_L)
def test_1_pairs_table(h, L):
    n = 0
    for par in pc.table():
        if par[0] != L:
            continue
        srcs = pc.synthetic(par, seed=n)
        src_a = pl.sources(len(srcs[0]), 4, n, FILLS); src_b = pl.sources(len(srcs[2]), 4, n + 1000, FILLS)
        d = [dev(x, t) for x, t in zip(srcs, (np.int32, np.int64, np.int32, np.int64))]
        d_a, d_b = [dev(s) for s in src_a], [dev(s) for s in src_b]
        nseq = len(srcs[1]) - 1
        pre = pairs_pre(h, d, len(srcs[0]), len(srcs[2]), nseq, par)
        base = None
        for (k, sides), (_, host_sides) in zip(pair_sides(n, d_a, d_b), pair_sides(n, src_a, src_b)):
            want = pl.restate_pair_planes(srcs[1], srcs[3], src_a=host_sides[0], src_b=host_sides[1], fill=FILLS[:k], **split(par))
            base = check("pairs", pre, L, nseq, want, sides, FILLS[:k], base=base)
        if n % 6 == 0:
            _, cls_id, sep_id, double_sep, mode, max_a, stride, max_rows, pad_left = par
            args = (L, cls_id, sep_id, pc.PAD, mode, max_a, stride, max_rows, pad_left, double_sep)
            got = bf.ids_to_pair_rows_planes_batch(h, *srcs, *args, src_a=host_sides[0], src_b=host_sides[1], fill=FILLS[:4])
            plain = bf.ids_to_pair_rows_batch(h, *srcs, *args)
            assert len(got) == 7 and all(np.array_equal(a, b) for a, b in zip(got[:6], plain))
            assert all(np.array_equal(g, w) for g, w in zip(got[6], want[0]))
        n += 1
    assert n > 0


# ---- 2. capacity
@pytest.mark.parametrize("par", [(8, rc.CLS, rc.SEP, 1, 0, False), (63, rc.CLS, -1, 1, 3, True), (64, rc.CLS, rc.SEP, 0, 0, False)])
def test_2_capacity_rows(h, par):
    L = par[0]
    ids, off = rc.synthetic(*rc.geometry(L, par[1], par[2], par[3]))
    src = pl.sources(len(ids), 3, 7, FILLS)
    want = pl.restate_planes(off, src=src, fill=FILLS[:3], **split(par))
    total, nseq = len(want[1]), len(off) - 1
    d_ids, d_off, d_src = dev(ids), dev(off, np.int64), [dev(s) for s in src]
    pre = rows_pre(h, d_ids, len(ids), d_off, nseq, par)
    for cap in (0, total - 1, total, total + 3):
        check("rows", pre, L, nseq, want, [d_src], FILLS[:3], cap=cap)                                         # bit 0 exactly when total > cap
        check("rows", pre, L, nseq, want, [d_src], FILLS[:3], cap=cap, ptake=[True, False, True])               # a NULL entry is skipped
        check("rows", pre, L, nseq, want, [d_src], FILLS[:3], cap=cap, take=[False] * 4, ptake=[False, True, False])   # one plane alone: the drop is reported
    check("rows", pre, L, nseq, want, [d_src], FILLS[:3], cap=0, take=[False] * 4, ptake=[False] * 3)           # the size query: complete offsets, no bit 0
    # host form: BF_E_CAPACITY with complete offsets and nothing else written; the size query needs no capacity
    hi, ho = np.ascontiguousarray(ids, dtype=np.int32), np.ascontiguousarray(off, dtype=np.int64)
    L_, cls_id, sep_id, stride, max_rows, pad_left = par
    hpre = (vp(h), hi.ctypes.data, ho.ctypes.data, nseq, L, cls_id, sep_id, rc.PAD, stride, max_rows, 1 if pad_left else 0)
    c_src = (vp * 3)(*[s.ctypes.data for s in src]); c_fill = (c_i32 * 3)(*FILLS[:3])
    for cap in (0, total - 1):
        outs = [np.full((cap, L), CANARY32, dtype=np.int32) for _ in range(3)]
        rows = np.full((cap, L), CANARY32, dtype=np.int32)
        r_off = np.full(nseq + 1, -1, dtype=np.int64)
        r = bf.lib().IdsToRowsPlanesBatch(*hpre, rows.ctypes.data, None, None, None, cap, r_off.ctypes.data, 3, c_src, c_fill, (vp * 3)(*[o.ctypes.data for o in outs]))
        assert r == E_CAPACITY and np.array_equal(r_off, want[3]) and (rows == CANARY32).all() and all((o == CANARY32).all() for o in outs)
    r_off = np.full(nseq + 1, -1, dtype=np.int64)
    assert bf.lib().IdsToRowsPlanesBatch(*hpre, None, None, None, None, 0, r_off.ctypes.data, 3, c_src, c_fill, (vp * 3)(None, None, None)) == total
    assert np.array_equal(r_off, want[3])
    outs = [np.full((total, L), CANARY32, dtype=np.int32) for _ in range(3)]                                    # one plane alone, no base output
    assert bf.lib().IdsToRowsPlanesBatch(*hpre, None, None, None, None, total, r_off.ctypes.data, 3, c_src, c_fill, (vp * 3)(None, outs[1].ctypes.data, None)) == total
    assert np.array_equal(outs[1], want[0][1]) and (outs[0] == CANARY32).all() and (outs[2] == CANARY32).all()


@pytest.mark.parametrize("par", [(8, pc.CLS, pc.SEP, False, 0, 2, 1, 0, False), (64, pc.CLS, pc.SEP, True, 0, 59, 0, 0, True), (64, pc.CLS, pc.SEP, False, 1, 0, 0, 1, False)])
def test_2_capacity_pairs(h, par):
    L = par[0]
    srcs = pc.synthetic(par)
    src_b = pl.sources(len(srcs[2]), 2, 3, FILLS)
    want = pl.restate_pair_planes(srcs[1], srcs[3], src_b=src_b, fill=FILLS[:2], **split(par))
    total, nseq = len(want[1]), len(srcs[1]) - 1
    d = [dev(x, t) for x, t in zip(srcs, (np.int32, np.int64, np.int32, np.int64))]
    sides = [None, [dev(s) for s in src_b]]
    pre = pairs_pre(h, d, len(srcs[0]), len(srcs[2]), nseq, par)
    for cap in (0, total - 1, total, total + 3):
        check("pairs", pre, L, nseq, want, sides, FILLS[:2], cap=cap)
        check("pairs", pre, L, nseq, want, sides, FILLS[:2], cap=cap, take=[False] * 5, ptake=[False, True])
    check("pairs", pre, L, nseq, want, sides, FILLS[:2], cap=0, take=[False] * 5, ptake=[False] * 2)


# ---- 3. alignment
@pytest.mark.parametrize("L", [64, 63])
def test_3_alignment(h, L):
    """plane bases 0, 4 and 16 bytes behind a 16-byte boundary, alone and one aligned beside one shifted: L = 64 takes the wide stores only where
    every taken plane is aligned, L = 63 never; the planes are the same everywhere and nothing around them changed"""
    import pointer_cases as pt
    par = (L, rc.CLS, rc.SEP, 3, 0, False)
    ids, off = rc.synthetic(*rc.geometry(L, rc.CLS, rc.SEP, 3))
    src = pl.sources(len(ids), 2, 11, FILLS)
    want = pl.restate_planes(off, src=src, fill=FILLS[:2], **split(par))
    total, nseq = len(want[1]), len(off) - 1
    d_ids, d_off = pt.place(np.ascontiguousarray(ids), 4, b"\xff", b"\xff"), pt.place(np.ascontiguousarray(off), 8, b"\xff", b"\xff")
    d_src = [pt.place(s, 4 * (k + 1), b"\xff", b"\xff") for k, s in enumerate(src)]
    r_off = torch.empty(nseq + 1, dtype=torch.int64, device="cuda")
    pre = rows_pre(h, d_ids.addr, len(ids), d_off.addr, nseq, par)
    for shifts in ((0, 0), (1, 1), (4, 4), (0, 1), (1, 0), (0, 4), (4, 0), (1, 4)):
        rooms = [pt.room(np.int32, total * L, s) for s in shifts]
        r = bf.lib().IdsToRowsPlanesBatchDevice(*pre, None, None, None, None, total, ptr(r_off), 2, ptr_array([p.addr for p in d_src], 2), (c_i32 * 2)(*FILLS[:2]),
                                                ptr_array([x.addr for x in rooms], 2), None)
        assert r == 0 and status(h) == 0
        for room, w in zip(rooms, want[0]):
            assert np.array_equal(room.fetch().result(), w.reshape(-1)), shifts
            room.untouched(total * L, "plane shifts %d %d" % shifts)
    assert np.array_equal(r_off.cpu().numpy(), want[3])
    for p in [d_ids, d_off] + d_src:
        p.verify("plane inputs")


# ---- 4. size edges
def ragged_random(nseq, seed, longest):
    rnd = np.random.RandomState(seed)
    lens = rnd.randint(0, longest, size=nseq)
    lens[rnd.randint(0, nseq, size=max(1, nseq // 50))] = 0
    return pc.ragged(lens, 1000)


@pytest.mark.parametrize("nseq", [1, 1023, 1024, 1025, 5000])
def test_4_counts_around_the_scan_tile(h, nseq):
    ids, off = ragged_random(nseq, nseq, 24)
    src = pl.sources(len(ids), 2, nseq, FILLS)
    rows_case(h, ids, off, (8, rc.CLS, rc.SEP, 1, 0, False), src, FILLS[:2])
    rows_case(h, ids, off, (12, rc.CLS, rc.SEP, 0, 2, True), src, FILLS[:2], take=[True, True, False, False])
    ids_a, off_a = pc.ragged([0 if q % 2 == 0 else 2 for q in range(nseq)], pc.A0)       # neighbours of different geometry
    par = (8, pc.CLS, pc.SEP, False, 0, 2, 1, 0, False)
    src_a = pl.sources(len(ids_a), 2, 5, FILLS)
    want = pl.restate_pair_planes(off_a, off, src_a=src_a, src_b=src, fill=FILLS[:2], **split(par))
    d = [dev(ids_a), dev(off_a, np.int64), dev(ids), dev(off, np.int64)]
    check("pairs", pairs_pre(h, d, len(ids_a), len(ids), nseq, par), 8, nseq, want, [[dev(s) for s in src_a], [dev(s) for s in src]], FILLS[:2])


def test_4_very_many_windows(h):
    """one sequence (and the B of one pair) of 200,000 ids at L = 8 among short ones: 10^5 windows are 10^5 rows like any others; with neither a
    row's item nor its first id taken the lanes have workspace for the first rows only and find the rest by their own search"""
    lens = [3, 0, 7, 200000, 1, 6, 9]
    ids, off = pc.ragged(lens, 1000)
    src = pl.sources(len(ids), 2, 1, FILLS)
    want = rows_case(h, ids, off, (8, rc.CLS, rc.SEP, 1, 0, False), src, FILLS[:2], take=[True, False, False, False])
    assert want[3][4] - want[3][3] > 39000
    ids_a, off_a = pc.ragged([3, 0, 2, 2, 1, 0, 5], pc.A0)
    par = (8, pc.CLS, pc.SEP, False, 0, 2, 1, 0, False)
    want = pl.restate_pair_planes(off_a, off, src_b=src, fill=FILLS[:2], **split(par))
    assert want[3][4] - want[3][3] == 1 + (200000 - 3 + 1) // 2
    d = [dev(ids_a), dev(off_a, np.int64), dev(ids), dev(off, np.int64)]
    check("pairs", pairs_pre(h, d, len(ids_a), len(ids), 7, par), 8, 7, want, [None, [dev(s) for s in src]], FILLS[:2], take=[False] * 5)


def test_4_more_lanes_than_one_pass_of_the_grid(h):
    """one-row sequences at L = 9 (the narrow form: a lane per cell) whose cells outnumber the lanes of the largest grid, 8 blocks of 256 per
    compute unit: the grid-stride step of k_rowstage_planes runs"""
    L = 9
    lanes = torch.cuda.get_device_properties(0).multi_processor_count * 8 * 256
    nseq = lanes // L + 8000
    assert nseq * L > lanes
    rnd = np.random.RandomState(9)
    ids, off = pc.ragged(rnd.randint(0, 12, size=nseq), 1000)
    src = pl.sources(len(ids), 2, 2, FILLS)
    want = pl.restate_planes_truncated(off, L, src, FILLS[:2])
    d_ids, d_off, d_src = dev(ids), dev(off, np.int64), [dev(s) for s in src]
    check("rows", rows_pre(h, d_ids, len(ids), d_off, nseq, (L, rc.CLS, rc.SEP, 0, 1, False)), L, nseq, want, [d_src], FILLS[:2], take=[False] * 4)


# ---- 5. hostile inputs
BAD = [([0, 5, 3, 12, 20], 60), ([0, 10, 70, 70, 80], 60), ([0, 10, 20, 35, 60], 30), ([-1, 4, 9, 12, 13], 60)]
GOOD = ([0, 3, 9, 9, 30], 60)


def test_5_bad_ranges(h):
    ids = (1000 + np.arange(60)).astype(np.int32)
    src = pl.sources(60, 2, 4, FILLS)
    for off, ids_len in BAD:
        want = rows_case(h, ids, off, (8, rc.CLS, rc.SEP, 1, 0, False), src, FILLS[:2], ids_len=ids_len)
        assert want[4] == 8
    ids_b = (pc.B0 + np.arange(60)).astype(np.int32)
    src_b = pl.sources(60, 2, 5, FILLS)
    d = [dev(ids), None, dev(ids_b), None]
    d_a, d_b = [dev(s) for s in src], [dev(s) for s in src_b]
    for par in ((8, pc.CLS, pc.SEP, False, 0, 2, 1, 0, False), (9, pc.CLS, pc.SEP, True, 1, 0, 0, 1, True)):
        for (oa, la), (ob, lb) in [(b, GOOD) for b in BAD] + [(GOOD, b) for b in BAD] + [(BAD[0], BAD[1]), (BAD[2], BAD[3])]:
            want = pl.restate_pair_planes(oa, ob, src_a=[s[:la] for s in src], src_b=[s[:lb] for s in src_b], fill=FILLS[:2], len_a=la, len_b=lb, **split(par))
            assert want[4] == 8
            d[1], d[3] = dev(oa, np.int64), dev(ob, np.int64)
            check("pairs", pairs_pre(h, d, la, lb, 4, par), par[0], 4, want, [d_a, d_b], FILLS[:2])


def test_5_both_sides_in_one_array(h):
    """ids and companion arrays shared by both sides: A the sequences as they are, B the sequences from the fourth on"""
    ids, off = pc.ragged([3, 0, 9, 4, 17, 1], pc.A0)
    src = pl.sources(len(ids), 2, 6, FILLS)
    off_b = np.concatenate([off[3:], off[-1:].repeat(3)])
    par = (10, pc.CLS, pc.SEP, False, 0, 3, 1, 0, False)
    want = pl.restate_pair_planes(off, off_b, src_a=src, src_b=src, fill=FILLS[:2], len_a=len(ids), len_b=len(ids), **split(par))
    d_ids, d_src = dev(ids), [dev(s) for s in src]
    d = [d_ids, dev(off, np.int64), d_ids, dev(off_b, np.int64)]
    check("pairs", pairs_pre(h, d, len(ids), len(ids), 6, par), 10, 6, want, [d_src, d_src], FILLS[:2])


def test_5_behind_a_tokenizer_call_that_overflowed(h):
    """TextToIdsWithOffsetsBatchDevice with a capacity too small, the planes call behind it on the same stream with ids_len = that capacity and
    no synchronisation between them: the documents that did not fit have no id cells, the others their exact offsets"""
    docs = [b"hello world again", b"unaffable telescope", b"a b c d e f g h i j k l m n o p", b"the end"]
    text, off = bf.pack_docs(docs)
    full, f_st, f_en, f_off = bf.text_to_ids_with_offsets_batch(h, (text, off), 64, 100)
    cap = int(f_off[2]) + 3                                    # documents 0 and 1 fit, 2 and 3 do not
    d_text, d_doc = torch.from_numpy(text.copy()).cuda(), torch.from_numpy(off).cuda()
    d_ids, d_st, d_en = (torch.full((cap,), -9, dtype=I32, device="cuda") for _ in range(3))
    d_off = torch.empty(5, dtype=torch.int64, device="cuda")
    assert bf.lib().TextToIdsWithOffsetsBatchDevice(vp(h), ptr(d_text), ptr(d_doc), 4, len(text), ptr(d_ids), ptr(d_st), ptr(d_en), cap, ptr(d_off), 64, 100, None) == 0
    got = bf.ids_to_rows_planes_batch_device(h, d_ids, d_off, 16, rc.CLS, rc.SEP, rc.PAD, 2, 0, src=[d_st, d_en], fill=[-1, -1])
    assert status(h) == 8 and np.array_equal(d_off.cpu().numpy(), f_off)
    want = pl.restate_planes(f_off, 16, rc.CLS, rc.SEP, 2, 0, False, [f_st[:cap], f_en[:cap]], [-1, -1], ids_len=cap)
    assert want[4] == 8 and len(want[1]) == int(got[4][-1].item())
    for g, w in zip(got[5], want[0]):
        assert np.array_equal(g.cpu().numpy(), w)
    assert (want[0][0][int(want[3][2]):] == -1).all() and (want[0][0][0][1:3] >= 0).all()


def test_5_refused_arguments(h):
    ids = torch.arange(4, dtype=I32, device="cuda"); off = torch.tensor([0, 4], dtype=torch.int64, device="cuda")
    r_off = torch.full((2,), -1, dtype=torch.int64, device="cuda")
    plane = torch.zeros(16, dtype=I32, device="cuda")
    L = bf.lib()
    fill2 = (c_i32 * 2)(-1, -1)

    def rows(nplanes=1, src=True, src0=True, fill=True, out=True, ids_len=4, hm=h):
        return L.IdsToRowsPlanesBatchDevice(vp(hm) if hm else None, ptr(ids), ids_len, ptr(off), 1 if ids_len else 0, 8, 1, 2, 0, 0, 1, 0, None, None, None, None, 2, ptr(r_off),
                                            nplanes, ptr_array([ids if src0 else None] * 2, 2) if src else None, fill2 if fill else None,
                                            ptr_array([plane, None], 2) if out else None, None)

    def pairs(nplanes=1, src_a=True, src_b=True, fill=True, out=True):
        return L.IdsToPairRowsPlanesBatchDevice(vp(h), ptr(ids), 4, ptr(off), ptr(ids), 4, ptr(off), 1, 8, 1, 2, 0, 1, 0, 0, 1, 0, None, None, None, None, None, 2, ptr(r_off),
                                                nplanes, ptr_array([ids, None], 2) if src_a else None, ptr_array([None, ids], 2) if src_b else None,
                                                fill2 if fill else None, ptr_array([plane, None], 2) if out else None, None)
    assert rows() == 0 and rows(nplanes=2) == 0 and rows(nplanes=0, src=False, fill=False, out=False) == 0
    assert rows(nplanes=-1) == E_ARG and rows(nplanes=5) == E_ARG and rows(fill=False) == E_ARG and rows(out=False) == E_ARG
    assert rows(src=False) == E_ARG and rows(src0=False) == E_ARG and rows(hm=None) == E_ARG
    assert rows(src=False, ids_len=0) == 0 and rows(src0=False, ids_len=0) == 0          # no id to read: no source needed
    assert pairs() == 0 and pairs(nplanes=2) == 0 and pairs(src_a=False) == 0 and pairs(src_b=False) == 0 and pairs(src_a=False, src_b=False) == 0
    assert pairs(nplanes=0, src_a=False, src_b=False, fill=False, out=False) == 0
    assert pairs(nplanes=-1) == E_ARG and pairs(nplanes=5) == E_ARG and pairs(fill=False) == E_ARG and pairs(out=False) == E_ARG
    # what the base call refuses, the planes call refuses
    assert L.IdsToRowsPlanesBatchDevice(vp(h), ptr(ids), 4, ptr(off), 1, 2, 1, 2, 0, 0, 1, 0, None, None, None, None, 2, ptr(r_off), 0, None, None, None, None) == E_ARG
    hi = np.arange(4, dtype=np.int32); ho = np.array([0, 4], dtype=np.int64); hr = np.zeros(2, dtype=np.int64); hp = np.zeros((1, 8), dtype=np.int32)
    hsrc = (vp * 1)(hi.ctypes.data); hout = (vp * 1)(hp.ctypes.data); hfill = (c_i32 * 1)(-1)

    def host(nplanes=1, src=hsrc, fill=hfill, out=hout):
        return L.IdsToRowsPlanesBatch(vp(h), hi.ctypes.data, ho.ctypes.data, 1, 8, 1, 2, 0, 0, 1, 0, None, None, None, None, 1, hr.ctypes.data, nplanes, src, fill, out)
    assert host() == 1 and hp[0].tolist() == [-1, 0, 1, 2, 3, -1, -1, -1]
    assert host(nplanes=5) == E_ARG and host(src=None) == E_ARG and host(src=(vp * 1)(None)) == E_ARG and host(fill=None) == E_ARG and host(out=None) == E_ARG

    s = torch.zeros(8, dtype=I32, device="cuda"); one = torch.zeros(1, dtype=I32, device="cuda")

    def span(hm=h, S=s, E=s, row_len=8, cap=1, nseq=1, first=one, last=one, so=one, eo=one):
        return L.RowsSpanCellsBatchDevice(vp(hm) if hm else None, ptr(S), ptr(E), row_len, cap, None, None, nseq, ptr(first), ptr(last), 0, ptr(so), ptr(eo), None)
    assert span() == 0 and span(row_len=1) == 0 and span(cap=0, S=None, E=None, first=None, last=None, so=None, eo=None) == 0 and span(nseq=0) == 0
    for bad in (dict(row_len=0), dict(row_len=-1), dict(row_len=(1 << 20) + 1), dict(cap=-1), dict(nseq=-1), dict(S=None), dict(E=None), dict(first=None),
                dict(last=None), dict(so=None), dict(eo=None), dict(hm=None)):
        assert span(**bad) == E_ARG, bad


def test_5_no_sequences(h):
    off = torch.zeros(1, dtype=torch.int64, device="cuda")
    got = call("rows", rows_pre(h, None, 0, off, 0, (8, rc.CLS, rc.SEP, 0, 1, False)), 8, 4, 0, None, ([[None, None]], FILLS[:2], [True, True]))
    assert got[0] == 0 and got[4] == 0 and got[2].tolist() == [0]
    assert all((b == (CANARY32 if b.dtype == np.int32 else CANARY8)).all() for b in got[1] + got[3])
    z32, z64 = np.zeros(0, dtype=np.int32), np.zeros(1, dtype=np.int64)
    out = bf.ids_to_rows_planes_batch(h, z32, z64, 8, rc.CLS, rc.SEP, src=[z32], fill=[-1])
    assert out[5][0].shape == (0, 8) and out[4].tolist() == [0]
    out = bf.ids_to_pair_rows_planes_batch(h, z32, z64, z32, z64, 8, pc.CLS, pc.SEP, src_b=[z32], fill=[-1])
    assert out[6][0].shape == (0, 8)


def test_5_handles_of_every_kind():
    import w2h_cases
    par = (8, rc.CLS, rc.SEP, 1, 0, False)
    ids, off = rc.synthetic(*rc.geometry(8, rc.CLS, rc.SEP, 1))
    src = pl.sources(len(ids), 2, 8, FILLS)
    kinds = []
    for path in (bfutil.model_path(bfutil.bert_model_name()), bfutil.model_path("gpt2.bin"), bfutil.model_path("bert_base_tok.i2w"), w2h_cases.FIXTURE):
        hm = bf.load_model(path)
        try:
            kinds.append(bf.lib().BfModelKind(vp(hm)))
            assert bf.lib().BfReserve(vp(hm), 64, 1 << 12, 0) == 0
            want = rows_case(hm, ids, off, par, src, FILLS[:2])
            S, E = dev(want[0][0]), dev(want[0][1])
            a = dev(np.zeros(len(off) - 1)); z = dev(np.full(len(off) - 1, 3))
            got = bf.rows_span_cells_device(hm, S.reshape(-1, 8), E.reshape(-1, 8), dev(want[1]), None, a, z, -100)
            ws, we, wst = pl.restate_span(want[0][0], want[0][1], want[1], len(off) - 1, np.zeros(len(off) - 1), np.full(len(off) - 1, 3), -100)
            assert status(hm) == wst and np.array_equal(got[0].cpu().numpy(), ws) and np.array_equal(got[1].cpu().numpy(), we)
        finally:
            bf.free_model(hm)
    assert kinds == [0, 3, 5, 6]                               # WordPiece, BPE, [i2w] only, [w2h] only


# ---- 6. span cells
SPAN_ROWS = {1: 1, 2: 70, 4: 70, 5: 7, 8: 300, 12: 70, 31: 33, 32: 64, 33: 65, 63: 100, 64: 129, 65: 17, 130: 50, 512: 9}


def window_planes(L, R, left):
    """monotone windows: row r holds k tokens from token t0 on behind one leading special, token t = bytes 4 t .. 4 t + 2 (byte 4 t + 3 is a gap);
    the padding in front in every other row when `left`; row 0 is all fill"""
    rnd = np.random.RandomState(L * 1000 + R)
    S = np.full((R, L), -1, dtype=np.int32); E = np.full((R, L), -1, dtype=np.int32)
    win = []
    for r in range(R):
        k = 0 if r == 0 else int(rnd.randint(0, L)) if L > 1 else 1
        t0 = int(rnd.randint(2, 50))
        at = L - k if (left and r % 2) else min(1, L - k)
        S[r, at:at + k] = 4 * (t0 + np.arange(k)); E[r, at:at + k] = 4 * (t0 + np.arange(k)) + 2
        win.append((t0, k))
    return S, E, win


def span_kinds(t0, k, kind):
    """a byte span relative to the window [t0, t0 + k): before it, behind it, in at the front, out at the back, exact edges, in gaps, none, inverted"""
    lo, hi = 4 * t0, 4 * (t0 + max(k, 1) - 1) + 2
    return [(lo - 8, lo - 5), (hi + 2, hi + 6), (lo - 3, lo + 1), (hi - 1, hi + 4), (lo, hi), (lo + 3, hi - 3 if hi - 3 >= lo + 3 else lo + 3), (-1, hi), (hi, lo - 1),
            (lo + 4, lo + 6), (lo, lo)][kind % 10]


def run_span(hm, S, E, row_seq, nseq, first, last, none, nrows=None):
    R, L = S.shape
    so, eo = (torch.full((R + 8,), CANARY32, dtype=I32, device="cuda") for _ in range(2))
    d_n = None if nrows is None else torch.tensor([nrows], dtype=torch.int64, device="cuda")
    d = [dev(S), dev(E), dev(row_seq), dev(first), dev(last)]
    r = bf.lib().RowsSpanCellsBatchDevice(vp(hm), ptr(d[0]), ptr(d[1]), L, R, ptr(d_n), ptr(d[2]), nseq, ptr(d[3]), ptr(d[4]), none, ptr(so), ptr(eo), None)
    assert r == 0
    st = status(hm)
    want = pl.restate_span(S, E, row_seq, nseq, first, last, none, nrows)
    for g, w in zip((so.cpu().numpy(), eo.cpu().numpy()), want[:2]):
        assert np.array_equal(g[:R], w), (L, R, nrows)
        assert (g[R:] == CANARY32).all()
    assert st == want[2]
    return want


@pytest.mark.parametrize("L", sorted(SPAN_ROWS))
def test_6_span_cells(h, L):
    R = SPAN_ROWS[L]
    for left in (False, True):
        S, E, win = window_planes(L, R, left)
        first = np.array([span_kinds(t0, k, r)[0] for r, (t0, k) in enumerate(win)], dtype=np.int32)
        last = np.array([span_kinds(t0, k, r)[1] for r, (t0, k) in enumerate(win)], dtype=np.int32)
        want = run_span(h, S, E, None, R, first, last, 0)                                  # row r is item r
        if R >= 20 and L >= 8:
            found = want[0] != want[1]
            assert found.any() and (want[0][~found] == 0).any()
        perm = np.random.RandomState(L).permutation(R).astype(np.int32)                    # items in another order than the rows
        run_span(h, S, E, perm, R, first[np.argsort(perm)], last[np.argsort(perm)], -100)
        seq = perm.copy(); seq[0] = R; seq[R // 2] = -1                                     # items out of range: bit 3
        assert run_span(h, S, E, seq, R, first, last, -100)[2] == 8
        for nrows in (0, R - 1, R + 5):                                                     # *d_nrows below / above rows_cap
            run_span(h, S, E, None, R, first, last, -100, nrows=nrows)
    rnd = np.random.RandomState(L + 7)                                                      # no order at all, a third of the cells without a token
    S = rnd.randint(0, 40, size=(R, L)).astype(np.int32); S[rnd.rand(R, L) < 0.33] = -1
    E = (np.maximum(S, 0) + rnd.randint(0, 6, size=(R, L))).astype(np.int32)
    first = rnd.randint(-2, 45, size=R).astype(np.int32); last = (first + rnd.randint(-1, 8, size=R)).astype(np.int32)
    run_span(h, S, E, None, R, first, last, -100)
    run_span(h, np.full((R, L), -1, dtype=np.int32), E, None, R, first, last, 0)            # every cell is fill


@pytest.mark.parametrize("L", [33, 8])
def test_6_more_span_groups_than_one_pass_of_the_grid(h, L):
    """more rows than the largest grid (8 blocks of 256 lanes per compute unit) has groups -- a wave per row at L = 33, eight lanes per row at L = 8: the
    grid-stride round of k_rows_span runs, with a last round in which some waves hold rows past the end; the row count comes from the device"""
    G = 64 if L > 32 else 8
    lanes = torch.cuda.get_device_properties(0).multi_processor_count * 8 * 256
    R = lanes // G + 1237
    assert R * G > lanes
    rnd = np.random.RandomState(L)
    k = rnd.randint(0, L, size=R)                                                          # tokens of row r: cells 1 .. k, from token t0 on (window_planes, as arrays)
    t0 = rnd.randint(2, 50, size=R)
    j = np.arange(L)[None, :]
    tok = (j >= 1) & (j <= k[:, None])
    S = np.where(tok, 4 * (t0[:, None] + j - 1), -1).astype(np.int32); E = np.where(tok, S + 2, -1).astype(np.int32)
    first = (4 * (t0 + rnd.randint(-2, 4, size=R)) + rnd.randint(0, 4, size=R)).astype(np.int32)
    last = (first + rnd.randint(-1, 12, size=R)).astype(np.int32)
    seq = rnd.permutation(R).astype(np.int32); seq[R - 1] = R                              # the last row's item is out of range
    so, eo = (torch.full((R + 8,), CANARY32, dtype=I32, device="cuda") for _ in range(2))
    d = [dev(S), dev(E), dev(seq), dev(first), dev(last)]
    for nrows in (R, R - 3):
        d_n = torch.tensor([nrows], dtype=torch.int64, device="cuda")
        so.fill_(CANARY32); eo.fill_(CANARY32)
        assert bf.lib().RowsSpanCellsBatchDevice(vp(h), ptr(d[0]), ptr(d[1]), L, R, ptr(d_n), ptr(d[2]), R, ptr(d[3]), ptr(d[4]), -100, ptr(so), ptr(eo), None) == 0
        st = status(h)
        want = pl.restate_span_array(S, E, seq, R, first, last, -100, nrows)
        assert st == want[2] == (8 if nrows == R else 0)
        for g, w in zip((so.cpu().numpy(), eo.cpu().numpy()), want[:2]):
            assert np.array_equal(g[:R], w) and (g[R:] == CANARY32).all(), (L, nrows)
    assert ((want[0] != -100) & (want[0] != CANARY32)).sum() > 300 and (want[0] == -100).sum() > 300          # (the inputs: hundreds of spans found, hundreds not)
    pick = np.concatenate([np.arange(64), np.arange(R - 64, R)])                           # the array form of the restatement against the loop, on a sample
    loop = pl.restate_span(S[pick], E[pick], seq[pick], R, first, last, -100)
    full = pl.restate_span_array(S, E, seq, R, first, last, -100)
    assert np.array_equal(loop[0], full[0][pick]) and np.array_equal(loop[1], full[1][pick])


def test_6_python_calls_refuse_what_the_kernels_would_misread(h):
    """a source, plane or row index that is not a contiguous int32 tensor on the device of the ids is refused, not read through its address"""
    ids, off = pc.ragged([3, 5], 1000)
    d_ids, d_off = dev(ids), dev(off, np.int64)
    labels64 = torch.arange(8, dtype=torch.int64, device="cuda")
    strided = torch.arange(16, dtype=I32, device="cuda")[::2]
    on_host = torch.arange(8, dtype=I32)
    for bad in (labels64, strided, on_host, np.arange(8, dtype=np.int32)):
        with pytest.raises(ValueError):
            bf.ids_to_rows_planes_batch_device(h, d_ids, d_off, 8, rc.CLS, rc.SEP, src=[bad], fill=[-1])
        with pytest.raises(ValueError):
            bf.ids_to_pair_rows_planes_batch_device(h, d_ids, d_off, d_ids, d_off, 16, pc.CLS, pc.SEP, src_a=[None], src_b=[bad], fill=[-1])
    *_, (plane,) = bf.ids_to_rows_planes_batch_device(h, d_ids, d_off, 8, rc.CLS, rc.SEP, src=[labels64.to(I32)], fill=[-1])
    assert plane.cpu().tolist() == [[-1, 0, 1, 2, -1, -1, -1, -1], [-1, 3, 4, 5, 6, 7, -1, -1]]
    ends = plane + 1
    span = (torch.tensor([1, 4], device="cuda"), torch.tensor([2, 8], device="cuda"))          # (int64 spans are converted: they are small per-item arrays)
    got = bf.rows_span_cells_device(h, plane, ends, None, None, *span)
    assert got[0].cpu().tolist() == [2, 2] and got[1].cpu().tolist() == [2, 5]
    for bad in (dict(starts=plane.to(torch.int64)), dict(ends=ends.t()), dict(row_seq=torch.zeros(2, dtype=torch.int64, device="cuda")),
                dict(row_offsets=torch.zeros(3, dtype=I32, device="cuda")), dict(starts=plane.reshape(-1), ends=ends.reshape(-1))):
        a = dict(dict(starts=plane, ends=ends, row_seq=None, row_offsets=None), **bad)
        with pytest.raises(ValueError):
            bf.rows_span_cells_device(h, a["starts"], a["ends"], a["row_seq"], a["row_offsets"], *span)


# ---- 7. text to tensors
def docs_on_device(docs):
    text, off = bf.pack_docs(docs)
    return text, off, torch.from_numpy(text.copy()).cuda(), torch.from_numpy(off).cuda()


@pytest.mark.parametrize("model", sorted(rc.ENCODE_MODELS))
def test_7_text_to_rows_with_offsets(model):
    sp = rc.ENCODE_MODELS[model]
    docs = rc.encode_docs()
    text, off, d_text, d_off = docs_on_device(docs)
    hm = bf.load_model(bfutil.model_path(model))
    try:
        for L, stride, max_rows, pad_left in rc.ENCODE_CASES:
            ids, st, en, id_off = bf.text_to_ids_with_offsets_batch(hm, (text, off), rc.encode_max_len(L, stride, max_rows), sp["unk"])
            want = pl.restate_planes(id_off, L, sp["cls_id"], sp["sep_id"], stride, max_rows, pad_left, [st, en], [-1, -1])
            rows = rc.restate(ids, id_off, L, sp["cls_id"], sp["sep_id"], sp["pad_id"], stride, max_rows, pad_left)
            args = (L, sp["cls_id"], sp["sep_id"], sp["pad_id"], sp["unk"], stride, max_rows, pad_left)
            got = bf.encode_batch_device(hm, d_text, d_off, *args, return_offsets=True)
            plain = bf.encode_batch_device(hm, d_text, d_off, *args)
            assert len(got) == 6 and len(plain) == 4 and status(hm) == 0
            for g, w in zip(got, (rows[0], rows[1], rows[2], rows[4], want[0][0], want[0][1])):
                assert tuple(g.shape) == w.shape and np.array_equal(g.cpu().numpy(), w), (L, stride)
            assert all(torch.equal(a, b) for a, b in zip(got[:4], plain))
        d_ids, d_st, d_en, d_id_off = bf.text_to_ids_with_offsets_batch_device(hm, d_text, d_off, 128, sp["unk"])          # the mirror of the host call
        ids, st, en, id_off = bf.text_to_ids_with_offsets_batch(hm, (text, off), 128, sp["unk"])
        n = len(ids)
        assert np.array_equal(d_id_off.cpu().numpy(), id_off)
        assert all(np.array_equal(g.cpu().numpy()[:n], w) for g, w in zip((d_ids, d_st, d_en), (ids, st, en)))
    finally:
        bf.free_model(hm)


@pytest.mark.parametrize("model", sorted(pc.ENCODE_MODELS))
def test_7_texts_to_pair_rows_with_offsets(model):
    sp = pc.ENCODE_MODELS[model]
    docs_a = rc.encode_docs()
    docs_b = [docs_a[pc.pair_partner(i, len(docs_a))] for i in range(len(docs_a))]
    ta, oa, d_ta, d_oa = docs_on_device(docs_a)
    tb, ob, d_tb, d_ob = docs_on_device(docs_b)
    hm = bf.load_model(bfutil.model_path(model))
    try:
        for L, mode, max_a, stride, max_rows, pad_left in pc.ENCODE_CASES:
            len_a, len_b = pc.encode_max_lens(L, mode, max_a, stride, max_rows)
            ia, sa, ea, fa = bf.text_to_ids_with_offsets_batch(hm, (ta, oa), len_a, sp["unk"])
            ib, sb, eb, fb = bf.text_to_ids_with_offsets_batch(hm, (tb, ob), len_b, sp["unk"])
            base = pc.restate(ia, fa, ib, fb, L, sp["cls_id"], sp["sep_id"], sp["pad_id"], mode, max_a, stride, max_rows, pad_left)
            args = (L, sp["cls_id"], sp["sep_id"], sp["pad_id"], sp["unk"], mode, max_a, stride, max_rows, pad_left)
            plain = bf.encode_pairs_batch_device(hm, d_ta, d_oa, d_tb, d_ob, *args)
            assert len(plain) == 6
            for both in (False, True):
                want = pl.restate_pair_planes(fa, fb, L, sp["cls_id"], sp["sep_id"], mode, max_a, stride, max_rows, pad_left, False, [sa, ea] if both else None, [sb, eb],
                                              [-1, -1])
                got = bf.encode_pairs_batch_device(hm, d_ta, d_oa, d_tb, d_ob, *args, return_offsets=True, offsets_a=both)
                assert len(got) == 8 and status(hm) == 0
                for g, w in zip(got, base[:6] + (want[0][0], want[0][1])):
                    assert tuple(g.shape) == w.shape and np.array_equal(g.cpu().numpy(), w), (L, mode, both)
                assert all(torch.equal(a, b) for a, b in zip(got[:6], plain))
    finally:
        bf.free_model(hm)


@pytest.mark.parametrize("model", sorted(pc.ENCODE_MODELS))
def test_7_questions_and_contexts_to_answer_cells(model):
    sp = pc.ENCODE_MODELS[model]
    docs = rc.encode_docs()
    ctx = sorted(docs, key=len)[-12:]                          # the longest documents: several windows each
    qs = [docs[(5 * i + 1) % len(docs)][:40] for i in range(len(ctx))]
    tq, oq, d_tq, d_oq = docs_on_device(qs)
    tc, oc, d_tc, d_oc = docs_on_device(ctx)
    L, max_q, stride = 32, 6, 5
    hm = bf.load_model(bfutil.model_path(model))
    try:
        iq, fq = bf.text_to_ids_batch(hm, (tq, oq), max_q, sp["unk"])
        ic, sc, ec, fc = bf.text_to_ids_with_offsets_batch(hm, (tc, oc), 2 ** 31 - 1, sp["unk"])
        # answers: the byte spans of known tokens -- tokens 3 k + 1 .. 3 k + 3 of context k (none where the context is that short), one without an answer
        a = np.full(len(ctx), -1, dtype=np.int32); z = np.full(len(ctx), -1, dtype=np.int32)
        for k in range(len(ctx) - 1):
            n = int(fc[k + 1] - fc[k])
            if n > 3 * k + 3:
                a[k], z[k] = sc[fc[k] + 3 * k + 1], ec[fc[k] + 3 * k + 3]
        base = pc.restate(iq, fq, ic, fc, L, sp["cls_id"], sp["sep_id"], sp["pad_id"], 0, max_q, stride, 0)
        want = pl.restate_pair_planes(fq, fc, L, sp["cls_id"], sp["sep_id"], 0, max_q, stride, 0, False, False, None, [sc, ec], [-1, -1])
        ws, we, wst = pl.restate_span(want[0][0], want[0][1], base[3], len(ctx), a, z, 0)
        assert wst == 0 and (ws != 0).sum() >= 3 and len(base[3]) > 2 * len(ctx)
        args = (d_tq, d_oq, d_tc, d_oc, L, sp["cls_id"], sp["sep_id"], sp["pad_id"], max_q, stride, sp["unk"])
        got = bf.encode_qa_batch_device(hm, *args, d_ans_first=dev(a), d_ans_last=dev(z))
        assert len(got) == 10 and status(hm) == 0
        for g, w in zip(got, base[:6] + (want[0][0], want[0][1], ws, we)):
            assert tuple(g.shape) == w.shape and np.array_equal(g.cpu().numpy(), w)
        assert len(bf.encode_qa_batch_device(hm, *args)) == 8
    finally:
        bf.free_model(hm)


# ---- 8. no allocation after BfReserve
def test_8_repeated_calls_after_reserve_allocate_nothing():
    """after BfReserve a repeated encode_qa_batch_device -- two tokenizer calls, the planes call, the span call -- leaves the device's free memory
    where it was (hipMemGetInfo): torch serves the outputs from its cache, the library's workspaces do not grow"""
    docs = rc.encode_docs() * 8
    qs = [d[:40] for d in docs]
    tq, oq, d_tq, d_oq = docs_on_device(qs)
    tc, oc, d_tc, d_oc = docs_on_device(docs)
    sp = pc.ENCODE_MODELS["bert_base_tok.bin"]
    hm = bf.load_model(bfutil.model_path("bert_base_tok.bin"))
    try:
        bf.reserve(hm, len(oc) - 1, max(len(tq), len(tc)), True)
        grows0 = bf.workspace_grows()
        ans = dev(np.full(len(docs), 4)), dev(np.full(len(docs), 9))
        args = (d_tq, d_oq, d_tc, d_oc, 32, sp["cls_id"], sp["sep_id"], sp["pad_id"], 6, 5, sp["unk"])
        a = bf.encode_qa_batch_device(hm, *args, d_ans_first=ans[0], d_ans_last=ans[1])
        torch.cuda.synchronize()
        assert bf.workspace_grows() == grows0, "the FIRST call on the reserved handle made the library allocate device memory (BfWorkspaceGrows)"
        a = [t.cpu().numpy() for t in a]
        free0 = torch.cuda.mem_get_info()[0]
        b = bf.encode_qa_batch_device(hm, *args, d_ans_first=ans[0], d_ans_last=ans[1])
        torch.cuda.synchronize()
        free1 = torch.cuda.mem_get_info()[0]
        assert free1 == free0, "the device's free memory moved by %d bytes across a reserved call" % (free0 - free1)
        assert bf.workspace_grows() == grows0, "the repeated call made the library allocate device memory (BfWorkspaceGrows)"
        for x, y in zip(a, b):
            assert np.array_equal(x, y.cpu().numpy())
        assert (a[8] != 0).any() and (a[6] >= 0).any()
    finally:
        bf.free_model(hm)
