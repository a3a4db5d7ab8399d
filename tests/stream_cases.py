"""TEST helpers for IdsToStreamRowsBatch: a restatement of the specification in include/blingfiretokdll_amd.h as a sequential program (written
from that text: the stream S is built as a Python list, unit after unit, and cut -- deliberately not the parallel formulation of
blingfire_amd/csrc/bf_stream.h: no scan, no search), a vectorised numpy restatement for device-size checks (the CPU tier holds it to the
sequential one), and the case tables the CPU and GPU tiers share."""
import itertools

import numpy as np

BOS, EOS, PAD, IGN = 1, 2, 0, -100
TABLE_L = [1, 2, 4, 5, 8, 64]
INT32_MAX = 2 ** 31 - 1
DROP_LAST, POS_FROM_ROW, LABELS_WITHIN = 1, 2, 4
CANARY = -0x35014542
# the order of the results of restate / restate_np, and of the ten NULL-able outputs of the Device call
NAMES = ("rows", "seg", "pos", "labels", "row_first_seq", "row_first_pos", "seq_row", "seq_col")


def bad_range(b, e, ids_len):
    return b < 0 or e < b or e > ids_len or e - b > INT32_MAX - 2


def restate(ids, off, L, bos=-1, eos=-1, pad=0, ignore=IGN, flags=0, ids_len=None, rows_cap=None, taken=True):
    """-> (rows, seg, pos, labels int32[R, L], row_first_seq, row_first_pos int32[R], seq_row, seq_col int32[nseq], R, T, status).
    The arrays are complete whatever rows_cap is (a caller compares what lies below min(R, rows_cap)); rows_cap and `taken` (a row output is
    taken) only decide status bit 0."""
    assert 1 <= L <= 1 << 20 and 0 <= flags < 8
    ids = np.asarray(ids, dtype=np.int32)
    off = [int(x) for x in off]
    nseq = len(off) - 1
    if ids_len is None:
        ids_len = len(ids)
    status = 0
    S, unit_of, place, seq_row, seq_col = [], [], [], [], []          # the stream; for every element its unit and its place there
    for q in range(nseq):
        b, e = off[q], off[q + 1]
        if bad_range(b, e, ids_len):                                  # an empty sequence, bit 3
            status |= 8
            tok = []
        else:
            tok = [int(x) for x in ids[b:e]]
        unit = ([bos] if bos >= 0 else []) + tok + ([eos] if eos >= 0 else [])
        seq_row.append(len(S) // L)
        seq_col.append(len(S) % L)
        for x, v in enumerate(unit):
            S.append(v); unit_of.append(q); place.append(x)
    T = len(S)
    R = T // L if flags & DROP_LAST else -(-T // L)
    rows = np.full((R, L), pad, dtype=np.int32)
    seg = np.zeros((R, L), dtype=np.int32)
    pos = np.zeros((R, L), dtype=np.int32)
    labels = np.full((R, L), ignore, dtype=np.int32)
    first_seq = np.zeros(R, dtype=np.int32)
    first_pos = np.zeros(R, dtype=np.int32)
    for r in range(R):
        f = unit_of[r * L]
        first_seq[r] = f
        first_pos[r] = place[r * L]
        for j in range(L):
            t = r * L + j
            if t >= T:
                break
            rows[r, j] = S[t]
            seg[r, j] = unit_of[t] - f + 1
            pos[r, j] = min(place[t], j) if flags & POS_FROM_ROW else place[t]
            if t + 1 < T and not (flags & LABELS_WITHIN and unit_of[t + 1] != unit_of[t]):
                labels[r, j] = S[t + 1]
    if rows_cap is not None and R > rows_cap and taken:
        status |= 1
    return (rows, seg, pos, labels, first_seq, first_pos, np.array(seq_row, dtype=np.int32), np.array(seq_col, dtype=np.int32), R, T, status)


def restate_np(ids, off, L, bos=-1, eos=-1, pad=0, ignore=IGN, flags=0, ids_len=None):
    """restate() for large inputs, in whole-array numpy operations; the same tuple"""
    ids = np.asarray(ids, dtype=np.int32)
    off = np.asarray(off, dtype=np.int64)
    nseq = len(off) - 1
    if ids_len is None:
        ids_len = len(ids)
    lead, trail = int(bos >= 0), int(eos >= 0)
    b, e = off[:-1], off[1:]
    bad = (b < 0) | (e < b) | (e > ids_len) | (e - b > INT32_MAX - 2)
    n = np.where(bad, 0, e - b)
    w = n + lead + trail
    W = np.zeros(nseq + 1, dtype=np.int64)
    np.cumsum(w, out=W[1:])
    T = int(W[-1])
    R = T // L if flags & DROP_LAST else -(-T // L)
    unit = np.repeat(np.arange(nseq, dtype=np.int64), w)             # the unit of every stream element
    x = np.arange(T, dtype=np.int64) - W[unit]
    S = np.empty(T, dtype=np.int32)
    is_bos = (x == 0) if lead else np.zeros(T, dtype=bool)
    is_eos = (x == w[unit] - 1) if trail else np.zeros(T, dtype=bool)
    is_id = ~(is_bos | is_eos)
    S[is_bos] = bos
    S[is_eos] = eos
    S[is_id] = ids[(np.where(bad, 0, b)[unit] + x - lead)[is_id]]
    cells = R * L
    k = min(cells, T)
    rows = np.full(cells, pad, dtype=np.int32); rows[:k] = S[:k]
    first_seq = unit[np.arange(R, dtype=np.int64) * L].astype(np.int32) if R else np.zeros(0, dtype=np.int32)
    first_pos = x[np.arange(R, dtype=np.int64) * L].astype(np.int32) if R else np.zeros(0, dtype=np.int32)
    seg = np.zeros(cells, dtype=np.int32)
    seg[:k] = (unit[:k] - np.repeat(first_seq.astype(np.int64), L)[:k] + 1).astype(np.int32)
    pos = np.zeros(cells, dtype=np.int32)
    j = np.arange(k, dtype=np.int64) % L
    pos[:k] = (np.minimum(x[:k], j) if flags & POS_FROM_ROW else x[:k]).astype(np.int32)
    labels = np.full(cells, ignore, dtype=np.int32)
    m = min(k, T - 1) if T else 0                                     # cells whose t + 1 < T
    lab = S[1:m + 1].copy()
    if flags & LABELS_WITHIN:
        lab[unit[1:m + 1] != unit[:m]] = ignore
    labels[:m] = lab
    status = 8 if bad.any() else 0
    return (rows.reshape(R, L), seg.reshape(R, L), pos.reshape(R, L), labels.reshape(R, L), first_seq, first_pos,
            (W[:-1] // L).astype(np.int32), (W[:-1] % L).astype(np.int32), R, T, status)


def same(a, b):
    """two results of restate / restate_np are equal"""
    return all(np.array_equal(x, y) and x.shape == y.shape for x, y in zip(a[:8], b[:8])) and tuple(a[8:]) == tuple(b[8:])


def table():
    """(L, bos, eos, flags) of the parameter table: every L with each special present and absent, all 8 flag values"""
    return [(L, b, e, fl) for L in TABLE_L for b, e in itertools.product((BOS, -1), (EOS, -1)) for fl in range(8)]


def ragged(lens, seed=0):
    """ragged ids of the given lengths (ids 1000.. so that no id equals a special, the padding or the ignored label)"""
    off = np.zeros(len(lens) + 1, dtype=np.int64)
    if len(lens):
        np.cumsum(lens, out=off[1:])
    return (1000 + seed + np.arange(int(off[-1]))).astype(np.int32), off


def tile_cases(tile_cells, stage_units, wide=True):
    """(name, lens, L, bos, eos) built from the fill kernel's tile geometry (cells per tile of the form that L selects, units a staged slice
    holds; wide = the form of four cells a lane, which row_len % 4 == 0 takes).  Without specials a sequence of n ids is a unit of width n."""
    tc, su = tile_cells, stage_units
    La, Lb = (4, 8) if wide else (5, 7)                           # a row_len that takes the form with this tile
    out = []
    for d in (-1, 0, 1):
        # the units of one tile's slice: one long unit up to the tile's edge region, then units of width 1 so that the slice of tile 1 holds su + d units
        # (the unit of 5 that the tile begins in, the units of width 1, the long unit behind them; where a tile is too short for that many
        # units of width 1, units of width 0 make up the count)
        k1 = min(su + d - 2, tc - 10)
        out.append(("staged%+d" % d, [tc - 3, 5] + [1] * k1 + [0] * (su + d - 2 - k1) + [3 * tc], La, -1, -1))
        # the same count reached with a run of units of width 0 inside the tile
        out.append(("zeros%+d" % d, [tc + 10] + [0] * (su + d - 5) + [1, 1, 2, tc], La, -1, -1))
        # a unit boundary exactly on a tile edge, and one cell to either side
        out.append(("edge%+d" % d, [tc + d, 7, tc - 7 - d, 9], La, -1, -1))
        out.append(("edge-specials%+d" % d, [tc + d - 2, 7, tc - 9 - d, 9], Lb, BOS, EOS))
    out.append(("three-tiles", [5, 3 * tc + 11, 6], La, -1, -1))
    out.append(("three-tiles-specials", [5, 3 * tc + 11, 6], Lb, BOS, EOS))
    out.append(("zero-run", [3] + [0] * 20000 + [2], La, -1, -1))
    out.append(("zero-run-start-end", [0] * 300 + [5, 0, 0, 7] + [0] * 300, La, -1, -1))
    out.append(("zero-run-start-end-long", [0] * (su + 50) + [tc, 1] + [0] * (su + 50), La, -1, -1))
    out.append(("long-row", [3 * tc + 5, 0, 9, 2 * tc], 2 * tc + (4 if wide else 5), BOS, EOS))
    out.append(("long-row-odd", [3 * tc + 5, 0, 9, 2 * tc], 2 * tc + (8 if wide else 3), -1, EOS))
    return out
