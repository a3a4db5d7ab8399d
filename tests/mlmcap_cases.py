"""TEST helpers for the capped MLM call (RowsMlmPredictionsBatchDevice), written from the specification in include/blingfiretokdll_amd.h and
from nothing else, on top of mlm_cases (its draw, eligibility and heads): selection straight from W(r, h)[0], the key of a unit as an exact
Python integer, f(h) by the loop of the definition; and the same over arrays for the large cases (a lexicographic sort of (W3, h) per row),
held to the loop on small inputs by the CPU tier."""
import numpy as np

import mlm_cases as mc

CANARY32 = mc.CANARY32
MAX_LEN = 4096
PROBS = (0.3, 0.8, 0.1)                                  # of the table cases
TABLE_SPECIALS = [mc.CLS, mc.SEP, mc.PAD]


def table_P(L):
    """the caps of the table cases: 1, 2, an eighth of the row, the row, more than the row"""
    return sorted({1, 2, max(1, L // 8), L, L + 5})


def selection(rows, mask=None, seg=None, S=None, E=None, special_ids=(), probs=mc.DEFAULT_PROBS, seed=0, epoch=0, row_base=0, heads_fn=None):
    """-> (h, selected, w3) over all rows: the head of every cell, selected = eligible and W(r, h)[0] < Ts, w3 = W(r, h)[3] (uint64 holding 32 bits)"""
    rows = np.asarray(rows, dtype=np.int32)
    R, L = rows.shape
    el = mc.eligible(rows, mask, seg, special_ids)
    h = (heads_fn or mc.heads)(el, S, E)
    r = np.arange(R, dtype=np.int64)[:, None] + np.int64(row_base) + np.zeros((1, L), dtype=np.int64)
    w0, _, _, w3 = mc.draw(r, h, seed, epoch)
    return h, el & (w0 < np.uint64(mc.thresholds(*probs)[0])), w3


def kept_loop(h, selected, w3, P):
    """the cap by the loop of the definition, keys and counts as Python ints -> kept bool[R, L]"""
    R, L = h.shape
    kept = np.zeros((R, L), dtype=bool)
    hl, sl, wl = h.tolist(), selected.tolist(), w3.tolist()
    for r in range(R):
        cells = [j for j in range(L) if sl[r][j]]
        key = {j: (int(wl[r][j]) << 32) | int(hl[r][j]) for j in cells}           # K(h(j)): the draw at the head and the head
        for j in cells:
            f = sum(1 for j2 in cells if key[j2] <= key[j])
            kept[r, j] = P == 0 or f <= P
    return kept


def kept_array(h, selected, w3, P):
    """kept_loop over arrays: per row a lexicographic sort of (W3, h) with the unselected cells behind; f of a cell = the cells up to the end
    of its run of equal keys"""
    R, L = h.shape
    if P == 0:
        return selected.copy()
    order = np.lexsort((h, w3.astype(np.int64), ~selected), axis=1)
    take = lambda a: np.take_along_axis(a, order, axis=1)
    sh, sw, ss = take(h), take(w3.astype(np.int64)), take(selected)
    last = np.ones((R, L), dtype=bool)
    last[:, :-1] = (sh[:, :-1] != sh[:, 1:]) | (sw[:, :-1] != sw[:, 1:]) | (ss[:, :-1] != ss[:, 1:])
    end = np.where(last, np.arange(1, L + 1, dtype=np.int64)[None, :], np.int64(L + 1))
    f = np.minimum.accumulate(end[:, ::-1], axis=1)[:, ::-1]
    kept = np.zeros((R, L), dtype=bool)
    np.put_along_axis(kept, order, ss & (f <= P), axis=1)
    return kept


def restate_cap(rows, mask=None, seg=None, S=None, E=None, special_ids=(), probs=mc.DEFAULT_PROBS, mask_id=mc.MASK, rand_range=mc.RAND_RANGE, ignore_label=-100,
                seed=0, epoch=0, nrows=None, row_base=0, max_pred=0, heads_fn=None, kept_fn=None):
    """-> (ids [R, L], labels [R, L], cells [R, P], pred_labels [R, P], count [R]) int32; rows at or past min(R, nrows) hold the canary.  With
    max_pred = 0 the three gathered outputs have width 0 (cells, pred_labels) and hold the uncapped count."""
    rows = np.asarray(rows, dtype=np.int32)
    R, L = rows.shape
    P = int(max_pred)
    n = R if nrows is None else max(0, min(R, int(nrows)))
    cut = lambda a: None if a is None else np.asarray(a)[:n]
    ids = np.full((R, L), CANARY32, dtype=np.int32); labels = np.full((R, L), CANARY32, dtype=np.int32)
    cells = np.full((R, P), CANARY32, dtype=np.int32); plabels = np.full((R, P), CANARY32, dtype=np.int32); count = np.full((R,), CANARY32, dtype=np.int32)
    if n == 0:
        return ids, labels, cells, plabels, count
    v = rows[:n]
    kw = dict(special_ids=special_ids, probs=probs, seed=seed, epoch=epoch, row_base=row_base, heads_fn=heads_fn)
    h, selected, w3 = selection(v, cut(mask), cut(seg), cut(S), cut(E), **kw)
    kept = (kept_fn or kept_loop)(h, selected, w3, P)
    assert not (kept & ~selected).any()
    # the action of a cell is the base call's: its own draw
    base_ids, base_labels = mc.restate_mlm(v, cut(mask), cut(seg), cut(S), cut(E), mask_id=mask_id, rand_range=rand_range, ignore_label=ignore_label, **kw)
    ids[:n] = np.where(kept, base_ids, v)
    labels[:n] = np.where(kept, v, np.int32(ignore_label))
    count[:n] = kept.sum(axis=1)
    if P > 0:
        assert (count[:n] <= P).all()
        cells[:n] = 0; plabels[:n] = ignore_label
        if kept_fn is None:                                   # the plain form
            for r in range(n):
                js = np.flatnonzero(kept[r])
                cells[r, :len(js)] = js
                plabels[r, :len(js)] = v[r, js]
        else:                                                 # over arrays: a stable sort brings the kept cells to the front in cell order
            W = min(P, L)
            order = np.argsort(~kept, axis=1, kind="stable")[:, :W]
            live = np.arange(W)[None, :] < count[:n, None]
            cells[:n, :W] = np.where(live, order, 0)
            plabels[:n, :W] = np.where(live, np.take_along_axis(v, order, axis=1), np.int32(ignore_label))
    return ids, labels, cells, plabels, count


def shares(rows, mask, seg, S, E, P, **kw):
    """of the rows: (binds, free, blocked) = the cap drops a unit / something is selected and all of it is kept / something is selected and
    nothing is kept"""
    h, selected, w3 = selection(rows, mask, seg, S, E, **kw)
    kept = kept_array(h, selected, w3, P)
    any_sel = selected.any(axis=1)
    binds = (selected & ~kept).any(axis=1)
    return binds.mean(), (any_sel & ~binds).mean(), (any_sel & ~kept.any(axis=1)).mean()


def table_inputs(L, R=257):
    """the rows and planes of the table cases: (rows, mask, seg, S, E)"""
    rows, mask, seg = mc.random_rows(R, L, L + R)
    S, E = mc.word_planes(R, L, L + R, long_units=L > 64)
    return rows, mask, seg, S, E
