"""TEST helpers for the companion planes (IdsToRowsPlanesBatch / IdsToPairRowsPlanesBatch) and the span cells (RowsSpanCellsBatchDevice), written
from the specification in include/blingfiretokdll_amd.h, not from blingfire_amd/csrc/bf_rows.h / bf_pairs.h.  The geometry of a row is not
restated a second time: the restatements of the base calls (rows_cases.restate, pair_cases.restate) lay out index-valued ids, and which
source element a cell holds is read back from the id it got."""
import numpy as np

import pair_cases
import rows_cases

BASE_A, BASE_B = 1 << 20, 1 << 29     # index-valued ids of side A (the only side of the rows form) and of side B: two ranges that meet neither
PAD_MARK = -7                         # each other nor a special; the padding id of the geometry runs (no id, no special)
MAX_PLANES = 4
CANARY32 = -0x35014542


def _index_ids(n, base):
    assert 0 <= n < BASE_B - BASE_A
    return (base + np.arange(n, dtype=np.int64)).astype(np.int32)


def _gather(cells, lo, hi, src, fill):
    """plane of `cells`: src[v - lo] where lo <= v < hi, else fill"""
    out = np.full(cells.shape, fill, dtype=np.int32)
    if src is not None:
        is_id = (cells >= lo) & (cells < hi)
        out[is_id] = np.asarray(src, dtype=np.int32)[cells[is_id].astype(np.int64) - lo]
    return out


def restate_planes(id_off, L, cls_id=-1, sep_id=-1, stride=0, max_rows=1, pad_left=False, src=(), fill=(), ids_len=None):
    """rows form -> (planes: list of int32[R, L], row_seq, row_first, row_offsets, status).  src[k]: an array parallel to the ids."""
    assert len(src) == len(fill) <= MAX_PLANES and cls_id < BASE_A and sep_id < BASE_A
    n = max([int(x) for x in id_off] + [0]) if ids_len is None else ids_len
    cells, _, seq, first, off, status = rows_cases.restate(_index_ids(n, BASE_A), id_off, L, cls_id, sep_id, PAD_MARK, stride, max_rows, pad_left, ids_len=n)
    return [_gather(cells, BASE_A, BASE_B, s, f) for s, f in zip(src, fill)], seq, first, off, status


def restate_planes_truncated(id_off, L, src, fill):
    """restate_planes(id_off, L, CLS, SEP, 0, 1, False, src, fill) over good ranges as array operations (rows_cases.restate_truncated, which
    tests/test_rows_host.py holds to the row form): for batches too large for the row-at-a-time form"""
    cells, _, seq, first, off = rows_cases.restate_truncated(_index_ids(int(id_off[-1]), BASE_A), id_off, L, rows_cases.CLS, rows_cases.SEP, PAD_MARK)
    return [_gather(cells, BASE_A, BASE_B, s, f) for s, f in zip(src, fill)], seq, first, off, 0


def restate_pair_planes(off_a, off_b, L, cls_id=-1, sep_id=-1, mode=0, max_a=0, stride=0, max_rows=1, pad_left=False, double_sep=False, src_a=None, src_b=None,
                        fill=(), len_a=None, len_b=None):
    """pairs form -> (planes, row_seq, row_first_b, row_offsets, status).  src_a / src_b: None, or a list with None entries allowed."""
    src_a = [None] * len(fill) if src_a is None else list(src_a)
    src_b = [None] * len(fill) if src_b is None else list(src_b)
    assert len(src_a) == len(src_b) == len(fill) <= MAX_PLANES
    na = max([int(x) for x in off_a] + [0]) if len_a is None else len_a
    nb = max([int(x) for x in off_b] + [0]) if len_b is None else len_b
    cells, _, _, seq, first, off, status = pair_cases.restate(_index_ids(na, BASE_A), off_a, _index_ids(nb, BASE_B), off_b, L, cls_id, sep_id, PAD_MARK, mode, max_a,
                                                              stride, max_rows, pad_left, double_sep, len_a=na, len_b=nb)
    planes = []
    for a, b, f in zip(src_a, src_b, fill):
        pa = _gather(cells, BASE_A, BASE_B, a, f)
        pb = _gather(cells, BASE_B, 1 << 31, b, f)
        planes.append(np.where((cells >= BASE_B), pb, pa).astype(np.int32))
    return planes, seq, first, off, status


def restate_span(S, E, row_seq, nseq, span_first, span_last, none_cell, nrows=None, canary=CANARY32):
    """-> (start_cell int32[R], end_cell int32[R], status); rows at or past nrows keep `canary`"""
    S = np.asarray(S); E = np.asarray(E)
    R, L = S.shape
    nrows = R if nrows is None else max(0, min(R, nrows))
    start = np.full(R, canary, dtype=np.int32); end = np.full(R, canary, dtype=np.int32)
    status = 0
    for r in range(nrows):
        q = r if row_seq is None else int(row_seq[r])
        start[r] = end[r] = none_cell
        if q < 0 or q >= nseq:
            status |= 8
            continue
        a, z = int(span_first[q]), int(span_last[q])
        lo = [j for j in range(L) if S[r, j] >= 0 and S[r, j] <= a]
        hi = [j for j in range(L) if S[r, j] >= 0 and E[r, j] >= z]
        if a >= 0 and z >= a and lo and hi:
            start[r], end[r] = max(lo), min(hi)
    return start, end, status


def restate_span_array(S, E, row_seq, nseq, span_first, span_last, none_cell, nrows=None, canary=CANARY32):
    """restate_span as array operations, for many rows (the tests hold it to the loop form on samples): the same arguments, the same result"""
    S = np.asarray(S); E = np.asarray(E)
    R, L = S.shape
    nrows = R if nrows is None else max(0, min(R, nrows))
    q = np.arange(R, dtype=np.int64) if row_seq is None else np.asarray(row_seq, dtype=np.int64)
    known = (q >= 0) & (q < nseq)
    qq = np.where(known, q, 0)
    first = np.asarray(span_first, dtype=np.int64); last = np.asarray(span_last, dtype=np.int64)
    a = first[qq] if len(first) else np.zeros(R, dtype=np.int64)
    z = last[qq] if len(last) else np.zeros(R, dtype=np.int64)
    has = S >= 0
    lo = has & (S <= a[:, None]); hi = has & (E >= z[:, None])
    found = known & (a >= 0) & (z >= a) & lo.any(axis=1) & hi.any(axis=1)
    start = np.where(found, L - 1 - np.argmax(lo[:, ::-1], axis=1), none_cell).astype(np.int32)
    end = np.where(found, np.argmax(hi, axis=1), none_cell).astype(np.int32)
    start[nrows:] = canary; end[nrows:] = canary
    return start, end, 8 if (~known[:nrows]).any() else 0


def sources(n, nplanes, seed, fills):
    """nplanes arrays of n elements parallel to the ids: small values around zero, negatives among them, and the plane's own fill among them too"""
    rnd = np.random.RandomState(seed)
    out = []
    for k in range(nplanes):
        s = rnd.randint(-50, 50, size=n).astype(np.int32)
        if n:
            s[rnd.randint(0, n, size=max(1, n // 5))] = fills[k]
        out.append(s)
    return out


FILLS = [-1, 0, -100, 7]
