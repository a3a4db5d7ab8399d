"""TEST helpers for the MLM masking call (RowsMlmMaskBatchDevice), written from the specification in include/blingfiretokdll_amd.h and from nothing
else: Philox4x32-10 as array operations in uint64, a plain loop for the head of every cell's unit, the decision rule with Python floats for
the thresholds; and the shapes and planes the CPU and GPU tiers share."""
import numpy as np

CANARY32 = 0x5A5A5A5A
M32 = np.uint64(0xFFFFFFFF)
PHILOX_M0, PHILOX_M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
PHILOX_W0, PHILOX_W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
S32 = np.uint64(32)

# (counter, key, output) of the specification
PHILOX_VECTORS = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
                  ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
                  ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]

CLS, SEP, PAD, MASK = 101, 102, 0, 103
RAND_RANGE = (1000, 30522)
TABLE_L = [1, 3, 4, 31, 32, 33, 64, 65, 130]          # the GPU tier; the CPU tier adds 200
DEFAULT_PROBS = (0.15, 0.8, 0.1)


def philox(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 over arrays (or scalars) of 32-bit values held in uint64 -> four uint64 arrays of 32-bit values"""
    c0, c1, c2, c3, k0, k1 = np.broadcast_arrays(*[np.asarray(x, dtype=np.uint64) for x in (c0, c1, c2, c3, k0, k1)])
    for _ in range(10):
        p0 = PHILOX_M0 * c0                               # (below 2^64: both factors are below 2^32)
        p1 = PHILOX_M1 * c2
        c0, c1, c2, c3 = (p1 >> S32) ^ c1 ^ k0, p1 & M32, (p0 >> S32) ^ c3 ^ k1, p0 & M32
        k0 = (k0 + PHILOX_W0) & M32
        k1 = (k1 + PHILOX_W1) & M32
    return c0, c1, c2, c3


def draw(r, j, seed, epoch):
    """W(r, j) for arrays r (row indices, any int64 >= 0) and j (cells)"""
    r = np.asarray(r, dtype=np.int64).astype(np.uint64)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return philox(r & M32, r >> S32, np.asarray(j, dtype=np.uint64), np.uint64(int(epoch) & 0xFFFFFFFF), np.uint64(seed & 0xFFFFFFFF), np.uint64(seed >> 32))


def thresholds(select_prob, mask_prob, random_prob):
    import math
    return tuple(int(math.floor(p * 4294967296.0)) for p in (select_prob, mask_prob, random_prob))


def eligible(rows, mask, seg, special_ids):
    el = np.ones(rows.shape, dtype=bool)
    if mask is not None:
        el &= np.asarray(mask) != 0
    if seg is not None:
        el &= np.asarray(seg) != 0
    for s in special_ids:
        el &= rows != s
    return el


def heads(el, S, E):
    """h(j) of every cell, by the loop of the definition (Python ints: no wrap at any value of the planes)"""
    R, L = el.shape
    h = np.tile(np.arange(L, dtype=np.int64), (R, 1))
    if S is None:
        return h
    el, S, E = el.tolist(), np.asarray(S).tolist(), np.asarray(E).tolist()
    for r in range(R):
        for j in range(1, L):
            if el[r][j - 1] and el[r][j] and S[r][j - 1] >= 0 and S[r][j] >= 0 and S[r][j] - 1 == E[r][j - 1]:
                h[r, j] = h[r, j - 1]
    return h


def heads_array(el, S, E):
    """heads() as array operations (the large cases): a running maximum of (continues ? -1 : j) along the row, in int64"""
    R, L = el.shape
    j = np.tile(np.arange(L, dtype=np.int64), (R, 1))
    if S is None:
        return j
    S = np.asarray(S, dtype=np.int64); E = np.asarray(E, dtype=np.int64)
    cont = np.zeros((R, L), dtype=bool)
    cont[:, 1:] = el[:, 1:] & el[:, :-1] & (S[:, 1:] >= 0) & (S[:, :-1] >= 0) & (S[:, 1:] - 1 == E[:, :-1])
    return np.maximum.accumulate(np.where(cont, -1, j), axis=1)


def restate_mlm(rows, mask=None, seg=None, S=None, E=None, special_ids=(), probs=DEFAULT_PROBS, mask_id=MASK, rand_range=RAND_RANGE, ignore_label=-100,
                seed=0, epoch=0, nrows=None, row_base=0, ids_init=None, labels_init=None, heads_fn=None):
    """-> (ids, labels) int32[R, L].  Rows at or past min(R, nrows) keep ids_init / labels_init (default: the canary).  row_base is added to
    the row index the generator sees (the host tier reaches rows above 2^32 that way); heads_fn = heads_array for the large cases."""
    rows = np.asarray(rows, dtype=np.int32)
    R, L = rows.shape
    n = R if nrows is None else max(0, min(R, int(nrows)))
    ids = np.full((R, L), CANARY32, dtype=np.int32) if ids_init is None else np.array(ids_init, dtype=np.int32).reshape(R, L)
    labels = np.full((R, L), CANARY32, dtype=np.int32) if labels_init is None else np.array(labels_init, dtype=np.int32).reshape(R, L)
    if n == 0:
        return ids, labels
    ts, tm, tr = thresholds(*probs)
    v = rows[:n]
    el = eligible(v, None if mask is None else np.asarray(mask)[:n], None if seg is None else np.asarray(seg)[:n], special_ids)
    h = (heads_fn or heads)(el, None if S is None else np.asarray(S)[:n], None if E is None else np.asarray(E)[:n])
    r = np.arange(n, dtype=np.int64)[:, None] + np.int64(row_base) + np.zeros((1, L), dtype=np.int64)
    j = np.tile(np.arange(L, dtype=np.int64), (n, 1))
    selected = el & (draw(r, h, seed, epoch)[0] < np.uint64(ts))
    _, w1, w2, _ = draw(r, j, seed, epoch)
    span = max(int(rand_range[1]) - int(rand_range[0]), 0)
    rand = (np.int64(rand_range[0]) + ((w2 * np.uint64(span)) >> S32).astype(np.int64)).astype(np.int32)
    to_mask = selected & (w1 < np.uint64(tm))
    to_rand = selected & ~to_mask & (w1 < np.uint64(tm + tr))
    ids[:n] = np.where(to_mask, np.int32(mask_id), np.where(to_rand, rand, v))
    labels[:n] = np.where(selected, v, np.int32(ignore_label))
    return ids, labels


def random_rows(R, L, seed, specials=(CLS, SEP, PAD)):
    """rows of ids in [1000, 30000) with specials sprinkled in, a right-padded mask and a segment plane with zeros at the padding"""
    rnd = np.random.RandomState(seed)
    rows = rnd.randint(1000, 30000, size=(R, L)).astype(np.int32)
    real = rnd.randint(0, L + 1, size=R)
    real[0] = L
    mask = (np.arange(L)[None, :] < real[:, None]).astype(np.uint8)
    rows[mask == 0] = PAD
    for s in specials:
        rows[rnd.rand(R, L) < 0.05] = s
    seg = np.where(mask != 0, 1 + (np.arange(L)[None, :] >= real[:, None] // 2), 0).astype(np.int32)
    return rows, mask, seg


def word_planes(R, L, seed, long_units=False):
    """synthetic offset planes: tokens of 1 .. 4 bytes, a token continues the one before it with probability 0.5 (0.9 with long_units: units
    that run over one and two chunk boundaries of 64 cells), a tenth of the cells hold no token (S = E = -1); row 0 is ONE unit from end to end"""
    rnd = np.random.RandomState(seed + 77)
    S = np.empty((R, L), dtype=np.int32); E = np.empty((R, L), dtype=np.int32)
    for r in range(R):
        at = 0
        for j in range(L):
            if r > 0 and rnd.rand() >= (0.9 if long_units else 0.5):
                at += 1 + int(rnd.randint(0, 3))          # a gap: the next token starts a new unit
            n = 1 + int(rnd.randint(0, 4))
            S[r, j], E[r, j] = at, at + n - 1
            at += n
    hole = rnd.rand(R, L) < 0.1
    hole[0] = False
    S[hole] = -1; E[hole] = -1
    return S, E


def unit_runs(h):
    """per row the list of (first, last) cells of every unit of more than one cell"""
    out = []
    for row in np.asarray(h):
        runs, j = [], 0
        while j < len(row):
            k = j
            while k + 1 < len(row) and row[k + 1] == row[j]:
                k += 1
            if k > j:
                runs.append((j, k))
            j = k + 1
        out.append(runs)
    return out
