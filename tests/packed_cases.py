"""TEST helpers for IdsToPackedRowsBatch: a restatement of the specification in include/blingfiretokdll_amd.h as the sequential greedy loop
(written from that text, one unit after the other -- deliberately not the parallel formulation of blingfire_amd/csrc/bf_packed.h: no
prefix sums, no next(), no doubling), and the case tables the CPU and GPU tiers share."""
import itertools

import numpy as np

CLS, SEP, PAD = 101, 102, 0
TABLE_L = [1, 4, 5, 8, 64]
INT32_MAX = 2 ** 31 - 1


def geometry(L, cls_id, sep_id):
    """body, or None when the call must answer BF_E_ARG"""
    body = L - (1 if cls_id >= 0 else 0) - (1 if sep_id >= 0 else 0)
    return body if 1 <= L <= 1 << 20 and body >= 1 else None


def restate(ids, off, L, cls=-1, sep=-1, pad=0, ids_len=None, rows_cap=None):
    """-> (rows int32[R, L], seg int32[R, L], pos int32[R, L], row_first_seq int32[R + 1], seq_row int32[nseq], seq_col int32[nseq], R, status).
    The arrays are complete whatever rows_cap is (a caller compares what lies below min(R, rows_cap)); rows_cap only decides status bit 0."""
    assert geometry(L, cls, sep) is not None
    body = geometry(L, cls, sep)
    ids = np.asarray(ids, dtype=np.int32)
    off = [int(x) for x in off]
    nseq = len(off) - 1
    if ids_len is None:
        ids_len = len(ids)
    rows, seg, pos, first, seq_row, seq_col, status = [], [], [], [], [], [], 0
    used = 0            # cells of the current row that are taken
    count = 0           # units in the current row
    for q in range(nseq):
        b, e = off[q], off[q + 1]
        if b < 0 or e < b or e > ids_len:                 # not inside [0, ids_len], or decreasing: an empty sequence, bit 3
            status |= 8
            tok = []
        else:
            tok = [int(x) for x in ids[b:min(e, b + body)]]
        unit = ([cls] if cls >= 0 else []) + tok + ([sep] if sep >= 0 else [])
        w = len(unit)
        if q == 0 or used + w > L:                        # the first unit opens row 0; a unit that does not fit opens the next row
            rows.append(np.full(L, pad, dtype=np.int32)); seg.append(np.zeros(L, dtype=np.int32)); pos.append(np.zeros(L, dtype=np.int32))
            first.append(q)
            used = count = 0
        count += 1
        seq_row.append(len(rows) - 1)
        seq_col.append(used)
        if w:
            rows[-1][used:used + w] = unit
            seg[-1][used:used + w] = count
            pos[-1][used:used + w] = np.arange(w)
        used += w
    R = len(rows)
    first.append(nseq)
    if rows_cap is not None and R > rows_cap:
        status |= 1
    stack = lambda a: np.stack(a) if a else np.zeros((0, L), dtype=np.int32)
    return (stack(rows), stack(seg), stack(pos), np.array(first, dtype=np.int32), np.array(seq_row, dtype=np.int32), np.array(seq_col, dtype=np.int32), R, status)


def table():
    """(L, cls_id, sep_id) of the parameter table: every L with each special present and absent, where a body of at least one id is left"""
    return [(L, c, s) for L in TABLE_L for c, s in itertools.product((CLS, -1), (SEP, -1)) if geometry(L, c, s) is not None]


def ragged(lens, seed=0):
    """ragged ids of the given lengths (ids 1000.. so that no id equals a special or the padding)"""
    off = np.zeros(len(lens) + 1, dtype=np.int64)
    if len(lens):
        np.cumsum(lens, out=off[1:])
    return (1000 + seed + np.arange(int(off[-1]))).astype(np.int32), off


def table_lengths(body):
    return [0, 1, body - 1, body, body + 1, 3 * body]


def synthetic(body, seed=0):
    """the table's lengths three times over in three orders, so that every length meets every other at a row's edge"""
    t = table_lengths(body)
    return ragged(t + t[::-1] + t[::2] + t[1::2] + [1, 1, 0, 0], seed)


def mixed(nseq, seed, L, cls=-1, sep=-1):
    """random lengths from empty to a little beyond the body, with runs of empty sequences"""
    body = geometry(L, cls, sep)
    rnd = np.random.RandomState(seed)
    lens = rnd.randint(0, body + 3, size=nseq)
    lens[rnd.rand(nseq) < 0.5] //= 4
    for start in rnd.randint(0, nseq, size=max(1, nseq // 40)):
        lens[start:start + rnd.randint(1, 6)] = 0
    return ragged(lens.tolist(), seed)


def exact_fit(L):
    """without specials: rows of two units whose widths add up to L exactly, alternating with pairs that add up to L + 1"""
    assert L >= 4
    lens = []
    for a in range(1, L - 1):
        lens += [a, L - a]                                # W[e] - W[s] == L: one row
        lens += [a, L - a + 1] if a > 1 else [L, 1]      # == L + 1: the second unit opens a row
    return ragged(lens)
