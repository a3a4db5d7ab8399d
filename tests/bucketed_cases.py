"""IdsToBucketedRowsBatch: the sequential restatement of the specification (include/blingfiretokdll_amd.h) and the parameter table of
tests/test_gpu_bucketed.py.  numpy alone."""
import functools

import numpy as np

CLS, SEP, PAD = 101, 102, 0
NSEQ = [0, 1] + [2 ** k + d for k in range(6, 13) for d in (-1, 0, 1)] + [3 * 4096 + 5]     # a wave, every tile size and its neighbours, several blocks
MAX_LENS = [200, 255, 256, 65535, 65536, 1 << 20]                                            # 1, 2 and 3 passes at their boundaries
PATTERNS = ["equal", "increasing", "two", "random", "empty", "bad"]
MULTIPLES = [1, 8, 64]


def up(x, multiple):
    return -(-x // multiple) * multiple


def restate(ids, off, max_len, cls, sep, pad, multiple, max_cells, max_rows=0, ids_len=None):
    """-> dict of rows, mask, order, seq_pos, first, len, cell (the arrays as the call writes them with exact caps), counts, status"""
    ids, off = np.asarray(ids, dtype=np.int32), np.asarray(off, dtype=np.int64)
    nseq, ids_len = len(off) - 1, len(ids) if ids_len is None else ids_len
    lead, trail = int(cls >= 0), int(sep >= 0)
    b, e = off[:-1], off[1:]
    bad = (b < 0) | (e < b) | (e > ids_len)
    k = np.where(bad, 0, np.minimum(e - b, max_len - lead - trail))
    w = lead + k + trail
    order = np.argsort(max_len - w, kind="stable").astype(np.int32)
    seq_pos = np.empty(nseq, dtype=np.int32)
    seq_pos[order] = np.arange(nseq, dtype=np.int32)
    first, lens, cell, rows, mask, i = [], [], [0], [], [], 0
    while i < nseq:
        L = max(multiple, up(int(w[order[i]]), multiple))
        j = min(nseq, i + max(1, min(max_cells // L, max_rows if max_rows > 0 else nseq)))
        first.append(i); lens.append(L); cell.append(cell[-1] + (j - i) * L)
        for q in order[i:j]:
            unit = [cls] * lead + ids[b[q]:b[q] + k[q]].tolist() + [sep] * trail
            rows += unit + [pad] * (L - len(unit)); mask += [1] * len(unit) + [0] * (L - len(unit))
        i = j
    return dict(rows=np.array(rows, dtype=np.int32), mask=np.array(mask, dtype=np.uint8), order=order, seq_pos=seq_pos,
                first=np.array(first + [nseq], dtype=np.int32), len=np.array(lens + [0], dtype=np.int32), cell=np.array(cell, dtype=np.int64),
                counts=np.array([len(first), cell[-1]], dtype=np.int64), status=8 if bad.any() else 0)


def ragged(nseq, max_len, pattern, seed=0):
    """-> (ids, offsets, ids_len, cls, sep) of one width pattern; above 65535 three sequences are long enough for the top digit to differ"""
    rng = np.random.default_rng(seed)
    n = {"equal": np.full(nseq, 5), "increasing": np.arange(nseq) // max(1, nseq // 1000), "two": np.where(np.arange(nseq) % 2, 3, 9),
         "random": rng.integers(0, 24, nseq), "empty": np.zeros(nseq, dtype=np.int64), "bad": rng.integers(1, 24, nseq)}[pattern].astype(np.int64)
    if max_len > 65535 and nseq >= 3 and pattern != "empty":
        n[[0, nseq // 2, nseq - 1]] = [70000, 66000, 140000]
    off = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
    ids = rng.integers(1000, 30000, int(off[-1])).astype(np.int32)
    ids_len = len(ids)
    if pattern == "bad" and nseq > 8:
        off[[5, 6]] = off[[6, 5]]                          # range 5 decreases
        ids_len = int(off[nseq - nseq // 4])               # the last quarter lies past ids_len
    return (ids, off, ids_len) + ((-1, -1) if pattern == "empty" else (CLS, SEP))


@functools.lru_cache(maxsize=None)
def case(nseq, max_len, pattern, multiple, budget, max_rows=0):
    """budget "min": the longest row is alone; "one": a single batch; else the cells.  -> (call arguments, the restatement)"""
    ids, off, ids_len, cls, sep = ragged(nseq, max_len, pattern, seed=nseq + max_len)
    widest = max(multiple, up(max_len, multiple))
    max_cells = widest if budget == "min" else max(widest, nseq * widest) if budget == "one" else max(widest, budget)
    args = dict(ids=ids, off=off, ids_len=ids_len, max_len=max_len, cls=cls, sep=sep, pad=PAD, multiple=multiple, max_cells=max_cells, max_rows=max_rows)
    return args, restate(ids, off, max_len, cls, sep, PAD, multiple, max_cells, max_rows, ids_len)
