"""TEST helpers for IdsToPairRowsBatch: a numpy restatement of the specification in include/blingfiretokdll_amd.h (written from that text, one
row at a time, not from blingfire_amd/csrc/bf_pairs.h; mode 1 drops one id at a time, as the text says, not by the closed form), and the
parameter table and pair lengths the CPU and GPU tiers share.  The end-to-end cases take their reference ids from the fixture of the rows
stage (tests/golden/rows/encode_ids.json through rows_cases)."""
import itertools

import numpy as np

import rows_cases

INT32_MAX = 2 ** 31 - 1
CLS, SEP, PAD = 101, 102, 0
A0, B0 = 1000, 500000                 # synthetic ids of A and of B: two ranges that meet neither each other nor a special
TABLE_L = [4, 5, 8, 63, 64, 130]


def specials(cls_id, sep_id, double_sep):
    """(lead, mid, trail) cells or None when the flags are refused"""
    if double_sep and sep_id < 0:
        return None
    return (1 if cls_id >= 0 else 0), (0 if sep_id < 0 else 2 if double_sep else 1), (1 if sep_id >= 0 else 0)


def room(L, cls_id, sep_id, double_sep):
    """T, the ids a row holds, or None when the call must answer BF_E_ARG for them"""
    sp = specials(cls_id, sep_id, double_sep)
    if sp is None or L < 1 or L > 1 << 20 or L - sum(sp) < 1:
        return None
    return L - sum(sp)


def accepted(L, cls_id, sep_id, double_sep, mode, max_a, stride, max_rows):
    T = room(L, cls_id, sep_id, double_sep)
    if T is None or mode not in (0, 1):
        return False
    if mode == 0:
        return 0 <= max_a <= T - 1 and 0 <= stride < T - max_a and max_rows >= 0
    return max_a == 0 and stride == 0 and max_rows == 1


def longest_first(na, nb, T):
    """(ka, kb): one id at a time from the end of the longer sequence, from B on a tie, until both fit"""
    ka, kb = na, nb
    while ka + kb > T:
        if ka > kb:
            ka -= 1
        else:
            kb -= 1
    return ka, kb


def _side(ids, off, q, ids_len):
    b, e = int(off[q]), int(off[q + 1])
    if b < 0 or e < b or e > ids_len:                     # not inside [0, len], or decreasing: that side is empty, bit 3
        return ids[:0], 8
    return ids[b:e], 0


def restate(ids_a, off_a, ids_b, off_b, L, cls_id=-1, sep_id=-1, pad_id=0, mode=0, max_a=0, stride=0, max_rows=1, pad_left=False, double_sep=False,
            len_a=None, len_b=None):
    """-> (rows int32[R, L], mask uint8[R, L], type uint8[R, L], row_seq int32[R], row_first_b int32[R], row_offsets int64[nseq+1], status)"""
    assert accepted(L, cls_id, sep_id, double_sep, mode, max_a, stride, max_rows)
    T = room(L, cls_id, sep_id, double_sep)
    ids_a = np.asarray(ids_a, dtype=np.int32); ids_b = np.asarray(ids_b, dtype=np.int32)
    len_a = len(ids_a) if len_a is None else len_a
    len_b = len(ids_b) if len_b is None else len_b
    lead = [cls_id] if cls_id >= 0 else []
    mid = [] if sep_id < 0 else [sep_id, sep_id] if double_sep else [sep_id]
    trail = [sep_id] if sep_id >= 0 else []
    rows, mask, types, seqs, firsts, offs, status = [], [], [], [], [], [0], 0
    for q in range(len(off_a) - 1):
        A, sa = _side(ids_a, off_a, q, len_a)
        B, sb = _side(ids_b, off_b, q, len_b)
        status |= sa | sb
        na, nb = len(A), len(B)
        if mode == 0:
            ka = min(na, max_a)
            body_b = T - ka
            step = body_b - stride
            nrows = 1 if nb <= body_b else 1 + -(-(nb - body_b) // step)
            if max_rows > 0:
                nrows = min(nrows, max_rows)
            wins = [(w * step, B[w * step:min(nb, w * step + body_b)]) for w in range(nrows)]
        else:
            ka, kb = longest_first(na, nb, T)
            wins = [(0, B[:kb])]
        for first, win in wins:
            first_half = lead + [int(x) for x in A[:ka]] + mid
            second_half = [int(x) for x in win] + trail
            real = first_half + second_half
            typ = [0] * len(first_half) + [1] * len(second_half)
            pad = L - len(real)
            assert pad >= 0
            rows.append([pad_id] * pad + real if pad_left else real + [pad_id] * pad)
            mask.append([0] * pad + [1] * len(real) if pad_left else [1] * len(real) + [0] * pad)
            types.append([0] * pad + typ if pad_left else typ + [0] * pad)
            seqs.append(q)
            firsts.append(min(first, INT32_MAX))
        offs.append(offs[-1] + len(wins))
    return (np.array(rows, dtype=np.int32).reshape(-1, L), np.array(mask, dtype=np.uint8).reshape(-1, L), np.array(types, dtype=np.uint8).reshape(-1, L),
            np.array(seqs, dtype=np.int32), np.array(firsts, dtype=np.int32), np.array(offs, dtype=np.int64), status)


def restate_one_row(ids_a, off_a, ids_b, off_b, L, cls_id, sep_id, pad_id, mode, max_a=0, chunk=1 << 16):
    """restate(...) for one row per pair (mode 1, or mode 0 with stride 0 and max_rows 1), both specials present, single separator, padding
    behind, good ranges, as array operations (for batches too large for the row-at-a-time form; tests/test_pairs_host.py holds it to that
    form): -> (rows, mask, type, row_seq, row_first_b, row_offsets).  Mode 1 is still the one-id-at-a-time loop, run on all pairs at once."""
    ids_a = np.asarray(ids_a, dtype=np.int32); ids_b = np.asarray(ids_b, dtype=np.int32)
    off_a = np.asarray(off_a, dtype=np.int64); off_b = np.asarray(off_b, dtype=np.int64)
    nseq, T = len(off_a) - 1, L - 3
    na, nb = np.diff(off_a), np.diff(off_b)
    if mode == 0:
        ka = np.minimum(na, max_a)
        kb = np.minimum(nb, T - ka)
    else:
        ka, kb = na.copy(), nb.copy()
        while True:
            over = ka + kb > T
            if not over.any():
                break
            from_a = over & (ka > kb)
            ka[from_a] -= 1
            kb[over & ~from_a] -= 1
    rows = np.empty((nseq, L), dtype=np.int32); mask = np.empty((nseq, L), dtype=np.uint8); typ = np.empty((nseq, L), dtype=np.uint8)
    j = np.arange(L, dtype=np.int64)[None, :]
    for lo in range(0, nseq, chunk):
        hi = min(nseq, lo + chunk)
        a, b = ka[lo:hi, None], kb[lo:hi, None]
        is_a = (j >= 1) & (j <= a)
        is_b = (j >= a + 2) & (j < a + 2 + b)
        is_sep = (j == a + 1) | (j == a + 2 + b)
        va = ids_a[np.where(is_a, off_a[lo:hi, None] + j - 1, 0)] if len(ids_a) else 0
        vb = ids_b[np.where(is_b, off_b[lo:hi, None] + j - a - 2, 0)] if len(ids_b) else 0
        r = np.where(is_a, va, np.where(is_b, vb, np.where(is_sep, sep_id, pad_id)))
        r[:, 0] = cls_id
        rows[lo:hi] = r
        mask[lo:hi] = j <= a + 2 + b
        typ[lo:hi] = (j >= a + 2) & (j <= a + 2 + b)
    return rows, mask, typ, np.arange(nseq, dtype=np.int32), np.zeros(nseq, dtype=np.int32), np.arange(nseq + 1, dtype=np.int64)


def table():
    """every parameter combination: (L, cls_id, sep_id, double_sep, mode, max_a, stride, max_rows, pad_left).  cls present / absent, sep
    absent / single / doubled; mode 0: max_a in {0, 1, the largest allowed}, stride in {0, 1, T - max_a - 1}, max_rows 0 .. 3, both padding
    sides; mode 1: both padding sides.  A combination the row has no room for is left out."""
    out = []
    for L in TABLE_L:
        for cls_id, (sep_id, double_sep) in itertools.product((CLS, -1), ((-1, False), (SEP, False), (SEP, True))):
            T = room(L, cls_id, sep_id, double_sep)
            if T is None:
                continue
            for pad_left in (False, True):
                out.append((L, cls_id, sep_id, double_sep, 1, 0, 0, 1, pad_left))
            for max_a in sorted({0, 1, T - 1}):
                for stride in sorted({0, 1, T - max_a - 1}):
                    for max_rows in (0, 1, 2, 3):
                        if not accepted(L, cls_id, sep_id, double_sep, 0, max_a, stride, max_rows):
                            continue
                        for pad_left in (False, True):
                            out.append((L, cls_id, sep_id, double_sep, 0, max_a, stride, max_rows, pad_left))
    return out


def pair_lengths(par):
    """the (na, nb) of a parameter set: mode 0 na in {0, 1, max_a - 1, max_a, max_a + 1} x nb around the windows of THAT pair's geometry;
    mode 1 the cross product of {0, 1, floor(T/2), ceil(T/2), ceil(T/2) + 1, T, T + 1, 3T}"""
    L, cls_id, sep_id, double_sep, mode, max_a, stride, max_rows, pad_left = par
    T = room(L, cls_id, sep_id, double_sep)
    if mode == 1:
        ns = [0, 1, T // 2, -(-T // 2), -(-T // 2) + 1, T, T + 1, 3 * T]
        return [(na, nb) for na in ns for nb in ns]
    out = []
    for na in (0, 1, max_a - 1, max_a, max_a + 1):
        if na < 0:
            continue
        body_b = T - min(na, max_a)
        step = body_b - stride
        out += [(na, nb) for nb in (0, 1, body_b - 1, body_b, body_b + 1, body_b + step, body_b + step + 1, 3 * body_b + 1)]
    return out


def ragged(lens, first_id):
    off = np.zeros(len(lens) + 1, dtype=np.int64)
    np.cumsum(lens, out=off[1:])
    return (first_id + np.arange(int(off[-1]))).astype(np.int32), off


def synthetic(par, seed=0):
    """(ids_a, off_a, ids_b, off_b) with the table's pair lengths under `par`"""
    lens = pair_lengths(par)
    ids_a, off_a = ragged([a for a, _ in lens], A0 + seed)
    ids_b, off_b = ragged([b for _, b in lens], B0 + seed)
    return ids_a, off_a, ids_b, off_b


def flags(pad_left, double_sep):
    return (1 if pad_left else 0) | (2 if double_sep else 0)


# ---- the end-to-end cases: A = document i, B = document (7 i + 3) mod n of rows_cases.encode_docs(), three specials; (L, mode, max_a, stride,
# max_rows, pad_left).  The max_len values encode_pairs_batch_device derives from them are keys of the rows fixture (6, 14, 2^31 - 1): mode 1 at
# L = 17 has T = 14 for both sides; mode 0 at L = 24 has max_a = 6 for A and every id for B.  (The third candidate, the same with max_rows = 1
# and left padding, derives T = 21 for B, which the fixture does not hold: it is not a case.)
ENCODE_CASES = [(17, 1, 0, 0, 1, False), (24, 0, 6, 4, 0, False)]


def encode_max_lens(L, mode, max_a, stride, max_rows, nspecials=3):
    """(max_len of A, max_len of B) of the chain"""
    T = L - nspecials
    if mode == 1:
        return T, T
    return max_a, (T + (max_rows - 1) * (T - stride) if max_rows > 0 else INT32_MAX)


def pair_partner(i, n):
    return (7 * i + 3) % n


def fixture_pairs(fx, model, len_a, len_b):
    """(ids_a, off_a, ids_b, off_b) of the stored reference answers: A = document i at max_len len_a, B = document (7 i + 3) mod n at len_b"""
    a = fx["models"][model][str(len_a)]
    b = fx["models"][model][str(len_b)]
    n = len(a)
    b = [b[pair_partner(i, n)] for i in range(n)]
    ids_a, off_a = np.array([x for d in a for x in d], dtype=np.int32), np.zeros(n + 1, dtype=np.int64)
    ids_b, off_b = np.array([x for d in b for x in d], dtype=np.int32), np.zeros(n + 1, dtype=np.int64)
    np.cumsum([len(d) for d in a], out=off_a[1:])
    np.cumsum([len(d) for d in b], out=off_b[1:])
    return ids_a, off_a, ids_b, off_b


ENCODE_MODELS = rows_cases.ENCODE_MODELS
