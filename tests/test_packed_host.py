"""CPU tier of IdsToPackedRowsBatch: the restatement of the specification (packed_cases.restate, the sequential greedy loop) pinned by
hand-written literal cases, its properties on random tables, and the lane code of blingfire_amd/csrc/bf_packed.h -- the code the kernels
run per lane -- compiled for the host (tests/hosttest/bf_packedtest.cpp) against the restatement on the same tables."""
import ctypes

import numpy as np
import pytest

import bfutil
import packed_cases as pc

c_i64, c_int, c_vp = ctypes.c_int64, ctypes.c_int, ctypes.c_void_p
C, S, P = pc.CLS, pc.SEP, pc.PAD
CANARY = -0x35014542


def lists(got):
    return [g.tolist() if hasattr(g, "tolist") else g for g in got]


# ---- 1. the restatement, pinned by literal cases (ids, offsets, L, cls, sep -> every output, written out by hand)
LITERAL = {
    "two units fill a row exactly": dict(
        ids=[11, 12, 13, 21, 22, 23, 31], off=[0, 3, 6, 7], L=6, cls=-1, sep=-1,
        rows=[[11, 12, 13, 21, 22, 23], [31, P, P, P, P, P]], seg=[[1, 1, 1, 2, 2, 2], [1, 0, 0, 0, 0, 0]], pos=[[0, 1, 2, 0, 1, 2], [0, 0, 0, 0, 0, 0]],
        first=[0, 2, 3], seq_row=[0, 0, 1], seq_col=[0, 3, 0]),
    "one id too many": dict(
        ids=[11, 12, 13, 21, 22, 23, 24], off=[0, 3, 7], L=6, cls=-1, sep=-1,
        rows=[[11, 12, 13, P, P, P], [21, 22, 23, 24, P, P]], seg=[[1, 1, 1, 0, 0, 0], [1, 1, 1, 1, 0, 0]], pos=[[0, 1, 2, 0, 0, 0], [0, 1, 2, 3, 0, 0]],
        first=[0, 1, 2], seq_row=[0, 1], seq_col=[0, 0]),
    "both specials; a truncated sequence": dict(
        ids=[11, 21, 22, 23, 24, 25, 26, 31], off=[0, 1, 7, 8], L=6, cls=C, sep=S,
        rows=[[C, 11, S, P, P, P], [C, 21, 22, 23, 24, S], [C, 31, S, P, P, P]], seg=[[1, 1, 1, 0, 0, 0], [1] * 6, [1, 1, 1, 0, 0, 0]],
        pos=[[0, 1, 2, 0, 0, 0], [0, 1, 2, 3, 4, 5], [0, 1, 2, 0, 0, 0]], first=[0, 1, 2, 3], seq_row=[0, 1, 2], seq_col=[0, 0, 0]),
    "an empty sequence with specials": dict(
        ids=[11, 31], off=[0, 1, 1, 2], L=8, cls=C, sep=S,
        rows=[[C, 11, S, C, S, C, 31, S]], seg=[[1, 1, 1, 2, 2, 3, 3, 3]], pos=[[0, 1, 2, 0, 1, 0, 1, 2]], first=[0, 3], seq_row=[0, 0, 0], seq_col=[0, 3, 5]),
    "an empty sequence without specials is counted by seg": dict(
        ids=[11, 31], off=[0, 1, 1, 2], L=4, cls=-1, sep=-1,
        rows=[[11, 31, P, P]], seg=[[1, 3, 0, 0]], pos=[[0, 0, 0, 0]], first=[0, 3], seq_row=[0, 0, 0], seq_col=[0, 1, 1]),
    "width-0 units at the end of a full row stay in it; at the end of the batch too": dict(
        ids=[11, 12, 13, 14, 21, 22], off=[0, 4, 4, 4, 6, 6, 6], L=4, cls=-1, sep=-1,
        rows=[[11, 12, 13, 14], [21, 22, P, P]], seg=[[1, 1, 1, 1], [1, 1, 0, 0]], pos=[[0, 1, 2, 3], [0, 1, 0, 0]],
        first=[0, 3, 6], seq_row=[0, 0, 0, 1, 1, 1], seq_col=[0, 4, 4, 0, 2, 2]),
    "an all-width-0 batch is one row of padding": dict(
        ids=[], off=[0, 0, 0, 0], L=4, cls=-1, sep=-1,
        rows=[[P, P, P, P]], seg=[[0, 0, 0, 0]], pos=[[0, 0, 0, 0]], first=[0, 3], seq_row=[0, 0, 0], seq_col=[0, 0, 0]),
    "no sequences": dict(ids=[], off=[0], L=4, cls=C, sep=S, rows=[], seg=[], pos=[], first=[0], seq_row=[], seq_col=[]),
    "L = 1": dict(
        ids=[11, 21, 22, 41], off=[0, 1, 3, 3, 4], L=1, cls=-1, sep=-1,
        rows=[[11], [21], [41]], seg=[[1], [1], [1]], pos=[[0], [0], [0]], first=[0, 1, 3, 4], seq_row=[0, 1, 1, 2], seq_col=[0, 0, 1, 0]),
    "cls alone": dict(
        ids=[11, 12, 21], off=[0, 2, 3], L=5, cls=C, sep=-1,
        rows=[[C, 11, 12, C, 21]], seg=[[1, 1, 1, 2, 2]], pos=[[0, 1, 2, 0, 1]], first=[0, 2], seq_row=[0, 0], seq_col=[0, 3]),
}


@pytest.mark.parametrize("name", sorted(LITERAL))
def test_restatement_literal(name):
    c = LITERAL[name]
    rows, seg, pos, first, seq_row, seq_col, R, status = pc.restate(c["ids"], c["off"], c["L"], c["cls"], c["sep"], P)
    assert R == len(c["rows"]) and status == 0
    assert rows.shape == seg.shape == pos.shape == (R, c["L"])
    assert lists((rows, seg, pos, first, seq_row, seq_col)) == [c["rows"], c["seg"], c["pos"], c["first"], c["seq_row"], c["seq_col"]]


def test_restatement_bad_range_and_capacity():
    # sequence 1 decreases, sequence 3 ends past ids_len: both are read as empty (their specials only), bit 3; R > rows_cap adds bit 0
    got = pc.restate([11, 12, 13, 14, 15, 16], [0, 2, 1, 4, 9], 4, C, -1, P, ids_len=6, rows_cap=1)
    assert lists(got) == [[[C, 11, 12, C], [C, 12, 13, 14], [C, P, P, P]], [[1, 1, 1, 2], [1, 1, 1, 1], [1, 0, 0, 0]], [[0, 1, 2, 0], [0, 1, 2, 3], [0, 0, 0, 0]],
                          [0, 2, 3, 4], [0, 0, 1, 2], [0, 3, 0, 0], 3, 9]


# ---- 2. properties on random tables
def random_tables():
    out = []
    for i, (L, cls, sep) in enumerate(pc.table()):
        for nseq in (1, 7, 200):
            out.append((L, cls, sep, nseq, 100 * i + nseq))
    return out


@pytest.mark.parametrize("L,cls,sep,nseq,seed", random_tables())
def test_properties(L, cls, sep, nseq, seed):
    ids, off = pc.mixed(nseq, seed, L, cls, sep)
    rows, seg, pos, first, seq_row, seq_col, R, status = pc.restate(ids, off, L, cls, sep, P)
    body, lead, trail = pc.geometry(L, cls, sep), int(cls >= 0), int(sep >= 0)
    w = [lead + min(int(off[q + 1] - off[q]), body) + trail for q in range(nseq)]
    assert status == 0 and R >= 1 and first[0] == 0 and first[R] == nseq and (np.diff(first) > 0).all()
    # every sequence is in exactly one row, and that row is the one whose range holds it
    assert all(first[seq_row[q]] <= q < first[seq_row[q] + 1] for q in range(nseq))
    for r in range(R):
        s, e = int(first[r]), int(first[r + 1])
        used = sum(w[s:e])
        assert used <= L                                  # no row is over-full
        if e < nseq and any(w[e:]):
            assert w[e] > 0 and used + w[e] > L           # greedy maximality; every row but row 0 begins with a unit of positive width
        # seg / pos / seq_col are consistent with rows
        assert (seg[r, used:] == 0).all() and (pos[r, used:] == 0).all() and (rows[r, used:] == P).all() and (seg[r, :used] > 0).all()
        for q in range(s, e):
            c = int(seq_col[q])
            assert c == sum(w[s:q])
            assert (seg[r, c:c + w[q]] == q - s + 1).all() and pos[r, c:c + w[q]].tolist() == list(range(w[q]))
            unit = ([cls] if lead else []) + ids[off[q]:off[q] + w[q] - lead - trail].tolist() + ([sep] if trail else [])
            assert rows[r, c:c + w[q]].tolist() == unit


# ---- 3. the lane code, compiled for the host, equals the restatement
@pytest.fixture(scope="module")
def ht():
    L = ctypes.CDLL(bfutil.HOSTTEST_LIB)
    L.bft_packed_batch.restype = c_i64
    L.bft_packed_batch.argtypes = [c_vp, c_i64, c_vp, c_i64] + [c_int] * 5 + [c_vp] * 4 + [c_i64, c_vp, c_vp, c_int, c_vp, ctypes.POINTER(c_int)]
    return L


def host_packed(ht, ids, off, L, cls, sep, rows_cap, ids_len=None, lane_cells=1, flags=0):
    """bft_packed_batch over canary-filled arrays of rows_cap rows -> (R, rows, seg, pos, first, seq_row, seq_col, status, next)"""
    ids = np.ascontiguousarray(ids, dtype=np.int32); off = np.ascontiguousarray(off, dtype=np.int64)
    nseq = len(off) - 1
    planes = [np.full((rows_cap, L), CANARY, dtype=np.int32) for _ in range(3)]
    first = np.full(rows_cap + 1, CANARY, dtype=np.int32)
    seq = [np.full(nseq, CANARY, dtype=np.int32) for _ in range(2)]
    nxt = np.full(nseq + 1, CANARY, dtype=np.int32)
    status = c_int(-1)
    R = ht.bft_packed_batch(ids.ctypes.data, len(ids) if ids_len is None else ids_len, off.ctypes.data, nseq, L, cls, sep, P, flags, *[p.ctypes.data for p in planes],
                            first.ctypes.data, rows_cap, seq[0].ctypes.data, seq[1].ctypes.data, lane_cells, nxt.ctypes.data, ctypes.byref(status))
    return (R, *planes, first, *seq, status.value, nxt)


def check_host(ht, ids, off, L, cls, sep, ids_len=None):
    want = pc.restate(ids, off, L, cls, sep, P, ids_len=ids_len)
    R = want[6]
    for cap in sorted({0, max(R - 1, 0), R, R + 3}):
        for lane_cells in ((1, 4) if L % 4 == 0 else (1,)):
            got = host_packed(ht, ids, off, L, cls, sep, cap, ids_len, lane_cells)
            key = (L, cls, sep, cap, lane_cells)
            k = min(cap, R)
            assert got[0] == R and got[7] == (want[7] | (1 if R > cap else 0)), key
            for g, w in zip(got[1:4], want[:3]):
                assert np.array_equal(g[:k], w[:k]) and (g[k:] == CANARY).all(), key
            assert np.array_equal(got[4][:k + 1], want[3][:k + 1]) and (got[4][k + 1:] == CANARY).all(), key
            assert np.array_equal(got[5], want[4]) and np.array_equal(got[6], want[5]), key
    return want


@pytest.mark.parametrize("L,cls,sep", pc.table())
def test_lane_code_equals_the_restatement(ht, L, cls, sep):
    body = pc.geometry(L, cls, sep)
    ids, off = pc.synthetic(body)
    check_host(ht, ids, off, L, cls, sep)
    for nseq in (1, 2, 3, 65, 300):
        ids, off = pc.mixed(nseq, nseq + L, L, cls, sep)
        check_host(ht, ids, off, L, cls, sep)


@pytest.mark.parametrize("name", sorted(LITERAL))
def test_lane_code_on_the_literal_cases(ht, name):
    c = LITERAL[name]
    check_host(ht, np.array(c["ids"], dtype=np.int32), c["off"], c["L"], c["cls"], c["sep"])


def test_lane_code_next_and_rounds(ht):
    """next(s) against its definition, on widths with runs of zeros; chains of every length around the powers of two (all units of width L:
    R = nseq, the longest chain there is) are marked completely by the rounds packed_rounds counts"""
    L = 8
    ids, off = pc.mixed(500, 3, L)
    got = host_packed(ht, ids, off, L, -1, -1, 0)
    W = np.concatenate([[0], np.cumsum(np.minimum(np.diff(off), L))])
    for s in range(500):
        assert got[8][s] == max(e for e in range(s + 1, 501) if W[e] - W[s] <= L), s
    assert got[8][500] == 500
    for nseq in list(range(1, 20)) + [31, 32, 33, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025]:
        ids, off = pc.ragged([L] * nseq)
        got = host_packed(ht, ids, off, L, -1, -1, 0)
        assert got[0] == nseq and got[5].tolist() == list(range(nseq)), nseq


def test_lane_code_exact_fit_and_width_zero_runs(ht):
    ids, off = pc.exact_fit(8)
    want = check_host(ht, ids, off, 8, -1, -1)
    w = np.diff(off)
    used = [int(w[want[3][r]:want[3][r + 1]].sum()) for r in range(want[6])]
    assert 8 in used and any(u + int(w[want[3][r + 1]]) == 9 for r, u in enumerate(used[:-1]))      # both sides of the boundary occur
    ids, off = pc.ragged([3] + [0] * 3000 + [2] + [0] * 50)
    want = check_host(ht, ids, off, 8, -1, -1)
    assert want[6] == 1 and want[1][0].tolist() == [1, 1, 1, 3002, 3002, 0, 0, 0]
    check_host(ht, ids, off, 8, C, S)


def test_lane_code_bad_ranges_and_refusals(ht):
    ids = (1000 + np.arange(60)).astype(np.int32)
    for off, ids_len in (([0, 5, 3, 12, 20], 60), ([0, 10, 70, 70, 80], 60), ([0, 10, 20, 35, 60], 30), ([-1, 4, 9], 60)):
        assert check_host(ht, ids, off, 8, C, S, ids_len=ids_len)[7] == 8
    for L, cls, sep, flags in ((0, -1, -1, 0), ((1 << 20) + 1, -1, -1, 0), (1, C, -1, 0), (2, C, S, 0), (8, C, S, 1), (8, C, S, -1)):
        st = c_int(0)
        one = np.array([0, 4], dtype=np.int64)
        assert ht.bft_packed_batch(ids.ctypes.data, 60, one.ctypes.data, 1, L, cls, sep, P, flags, None, None, None, None, 0, None, None, 1, None, ctypes.byref(st)) == -1, (L, cls, sep, flags)
