"""TEST helpers for the span-corruption call (RowsDenoiseBatchDevice), written from the specification in include/blingfiretokdll_amd.h and from
nothing else, on top of mlm_cases (its Philox, draw and eligibility): a sequential loop that follows the definition literally -- for every cell
it looks back for a start that still covers it, then it walks the row building the two rows as Python lists; the same over arrays for the large
cases, held to the loop by the CPU tier; and the case table the CPU and GPU tiers share, with what each case is in the table for."""
import functools
import math

import numpy as np

import mlm_cases as mc

CANARY32 = mc.CANARY32
NAMES = ("enc", "enc_cell", "enc_count", "dec", "dec_cell", "dec_count", "span_count")
TABLE_L = [1, 2, 3, 4, 5, 8, 9, 31, 32, 33, 63, 64, 65, 128, 129]          # the GPU tier; the CPU tier adds 200
HOST_L = TABLE_L + [200]
EOS, PAD = 1, 0
SPECIALS = [EOS, PAD, mc.SEP]
T5 = dict(sentinel_first=32099, sentinel_step=-1, max_sentinels=100)
DEFAULTS = dict(special_ids=(), start_prob=0.15, len_lo=1, len_hi=5, eos_id=EOS, pad_id=PAD, ignore_label=-100, seed=0, epoch=0, **T5)


def spec_of(kw):
    s = dict(DEFAULTS)
    s.update(kw)
    return s


def cells_of(rows, mask, seg, s, row_base=0):
    """per cell of [R, L]: present, eligible, starts, length (int64)"""
    rows = np.asarray(rows, dtype=np.int32)
    R, L = rows.shape
    present = mc.eligible(rows, mask, seg, ())
    el = mc.eligible(rows, mask, seg, s["special_ids"])
    r = np.arange(R, dtype=np.int64)[:, None] + np.int64(row_base) + np.zeros((1, L), dtype=np.int64)
    j = np.tile(np.arange(L, dtype=np.int64), (R, 1))
    w0, w1, _, _ = mc.draw(r, j, s["seed"], s["epoch"])
    ts = int(math.floor(s["start_prob"] * 4294967296.0))
    starts = el & (w0 < np.uint64(ts))
    length = np.int64(s["len_lo"]) + ((w1 * np.uint64(s["len_hi"] - s["len_lo"] + 1)) >> mc.S32).astype(np.int64)
    return present, el, starts, length


def raw_noise_loop(el, starts, length, len_hi):
    """the definition: cell j is raw noise iff it is eligible and some h <= j starts, with every cell of [h, j] eligible and h + len(h) > j"""
    R, L = el.shape
    raw = np.zeros((R, L), dtype=bool)
    e, s, n = el.tolist(), starts.tolist(), length.tolist()
    for r in range(R):
        for j in range(L):
            h = j
            while h >= 0 and e[r][h] and j - h < len_hi:      # (a start further back is too short whatever it drew: len <= len_hi)
                if s[r][h] and h + n[r][h] > j:
                    raw[r, j] = True
                    break
                h -= 1
    return raw


def raw_noise_array(el, starts, length, len_hi):
    """raw_noise_loop over arrays: a running maximum of the reaches that restarts behind every ineligible cell (the stretch's number in the high bits)"""
    R, L = el.shape
    j = np.tile(np.arange(L, dtype=np.int64), (R, 1))
    reach = np.where(starts, j + length, 0)
    stretch = np.cumsum(~el, axis=1).astype(np.int64) << np.int64(24)         # (a reach is below 2^22)
    v = np.maximum.accumulate(stretch + reach, axis=1) - stretch
    return el & (v > j)


def restate_denoise(rows, mask=None, seg=None, nrows=None, row_base=0, enc_len=None, dec_len=None, array=False, **kw):
    """-> a dict: the seven outputs (NAMES; rows at or past min(R, nrows) hold the canary), `status` (bit 0: a row is longer than enc_len / dec_len),
    and what the coverage checks read: present, eligible, starts, length, raw, noise, run (the run index of a raw-noise cell, -1 elsewhere).
    enc_len None = L, dec_len None = L + 2.  array=True: the array form (the large cases)."""
    s = spec_of(kw)
    rows = np.asarray(rows, dtype=np.int32)
    R, L = rows.shape
    EL = L if enc_len is None else int(enc_len)
    DL = L + 2 if dec_len is None else int(dec_len)
    n = R if nrows is None else max(0, min(R, int(nrows)))
    cut = lambda a: None if a is None else np.asarray(a)[:n]
    out = dict(enc=np.full((R, EL), CANARY32, dtype=np.int32), enc_cell=np.full((R, EL), CANARY32, dtype=np.int32), enc_count=np.full((R,), CANARY32, dtype=np.int32),
               dec=np.full((R, DL), CANARY32, dtype=np.int32), dec_cell=np.full((R, DL), CANARY32, dtype=np.int32), dec_count=np.full((R,), CANARY32, dtype=np.int32),
               span_count=np.full((R,), CANARY32, dtype=np.int32), status=0)
    if n == 0:
        return out
    v = rows[:n]
    present, el, starts, length = cells_of(v, cut(mask), cut(seg), s, row_base)
    raw = (raw_noise_array if array else raw_noise_loop)(el, starts, length, s["len_hi"])
    first, step, cap = s["sentinel_first"], s["sentinel_step"], s["max_sentinels"]
    eos = -1 if s["eos_id"] is None else int(s["eos_id"])
    out["enc"][:n] = s["pad_id"]; out["dec"][:n] = s["ignore_label"]; out["enc_cell"][:n] = -1; out["dec_cell"][:n] = -1
    if array:
        begin0 = raw.copy()
        begin0[:, 1:] &= ~raw[:, :-1]
        run = np.where(raw, np.cumsum(begin0, axis=1) - 1, -1)
        noise = raw & (run < cap)
        keep = present & ~noise
        begin = begin0 & noise
        ex = lambda a: np.cumsum(a, axis=1) - a                # the count in front of a cell
        epos = ex(keep) + ex(begin)
        dsent = ex(noise) + ex(begin)
        dpos = dsent + begin
        sent = (first + run * step).astype(np.int32)
        cell = np.tile(np.arange(L, dtype=np.int32), (n, 1))
        ne = keep.sum(axis=1) + begin.sum(axis=1)
        nd = noise.sum(axis=1) + begin.sum(axis=1) + (1 if eos >= 0 else 0)
        for sel, pos, width, ids_to, cell_to, ids, cells in ((keep, epos, EL, "enc", "enc_cell", v, cell), (begin, epos, EL, "enc", "enc_cell", sent, -1),
                                                             (begin, dsent, DL, "dec", "dec_cell", sent, -1), (noise, dpos, DL, "dec", "dec_cell", v, cell)):
            rr, jj = np.nonzero(sel & (pos < width))
            out[ids_to][rr, pos[rr, jj]] = ids[rr, jj]
            out[cell_to][rr, pos[rr, jj]] = -1 if isinstance(cells, int) else cells[rr, jj]
        if eos >= 0:
            rr = np.flatnonzero(nd - 1 < DL)
            out["dec"][rr, nd[rr] - 1] = eos
        out["enc_count"][:n] = ne; out["dec_count"][:n] = nd; out["span_count"][:n] = begin.sum(axis=1)
    else:
        run = np.full((n, L), -1, dtype=np.int64)
        noise = np.zeros((n, L), dtype=bool)
        ids, rw, pr = v.tolist(), raw.tolist(), present.tolist()
        for r in range(n):
            k = -1
            enc, enc_cell, dec, dec_cell = [], [], [], []
            for j in range(L):
                if rw[r][j]:
                    begins = j == 0 or not rw[r][j - 1]
                    if begins:
                        k += 1
                    run[r, j] = k
                    if k < cap:
                        noise[r, j] = True
                        if begins:
                            enc.append(first + k * step); enc_cell.append(-1)
                            dec.append(first + k * step); dec_cell.append(-1)
                        dec.append(ids[r][j]); dec_cell.append(j)
                        continue
                if pr[r][j]:
                    enc.append(ids[r][j]); enc_cell.append(j)
            if eos >= 0:
                dec.append(eos); dec_cell.append(-1)
            out["enc_count"][r] = len(enc); out["dec_count"][r] = len(dec); out["span_count"][r] = min(k + 1, cap)
            for name, lst, width in (("enc", enc, EL), ("enc_cell", enc_cell, EL), ("dec", dec, DL), ("dec_cell", dec_cell, DL)):
                m = min(len(lst), width)
                out[name][r, :m] = lst[:m]
    if (out["enc_count"][:n] > EL).any() or (out["dec_count"][:n] > DL).any():
        out["status"] = 1
    out.update(present=present, eligible=el, starts=starts, length=length, raw=raw, noise=noise, run=run)
    return out


def runs_of(flags):
    """per row the list of (first, last) cells of every maximal stretch of set flags"""
    out = []
    for row in np.asarray(flags).tolist():
        runs, j, L = [], 0, len(row)
        while j < L:
            if row[j]:
                k = j
                while k + 1 < L and row[k + 1]:
                    k += 1
                runs.append((j, k))
                j = k + 1
            else:
                j += 1
        out.append(runs)
    return out


# ---- the case table.  A case: name, rows, mask, seg and the keywords of the call (enc_len / dec_len among them where it truncates)
def stretch_rows(R, L, seed, every):
    """ids with an ineligible cell (SEP) every `every` cells, at a phase that moves with the row"""
    rnd = np.random.RandomState(seed)
    rows = rnd.randint(1000, 30000, size=(R, L)).astype(np.int32)
    for r in range(R):
        rows[r, (r % every)::every] = mc.SEP
    return rows


def packed_rows(R, L, seed):
    """rows in the layout of the packed call: sequences closed by SEP, a segment plane that numbers them from 1, zeros and PAD behind the last one"""
    rnd = np.random.RandomState(seed)
    rows = rnd.randint(1000, 30000, size=(R, L)).astype(np.int32)
    seg = np.zeros((R, L), dtype=np.int32)
    for r in range(R):
        at, k = 0, 1
        while at < L and (k == 1 or rnd.rand() < 0.8):
            n = min(L - at, 1 + int(rnd.randint(0, max(2, L // 2))))
            seg[r, at:at + n] = k
            rows[r, at + n - 1] = mc.SEP
            at += n; k += 1
        rows[r, at:] = PAD
    return rows, seg


def left_padded(R, L, seed):
    rows, mask, _ = mc.random_rows(R, L, seed)
    return rows[:, ::-1].copy(), mask[:, ::-1].copy()


def cases_for(L):
    R = 12 if L < 63 else 20
    out = []
    add = lambda name, rows, mask=None, seg=None, **kw: out.append(dict(name="%s/L%d" % (name, L), L=L, rows=rows, mask=mask, seg=seg, kw=kw))
    rows, mask, seg = mc.random_rows(R, L, 100 + L)
    mask[1] = 0; rows[1] = PAD; seg[1] = 0                     # a row of padding only
    plain = np.random.RandomState(200 + L).randint(1000, 30000, size=(R, L)).astype(np.int32)
    add("mixed", rows, mask, seg, special_ids=SPECIALS, start_prob=0.25, seed=11 * L + 1, epoch=1)
    add("plain", plain, special_ids=(), start_prob=0.1, len_lo=2, len_hi=4, sentinel_first=30000, sentinel_step=1, max_sentinels=1000, eos_id=None, seed=11 * L + 2)
    add("dense", plain, special_ids=(), start_prob=0.5, len_lo=1, len_hi=3, seed=11 * L + 3)
    add("none", rows, mask, seg, special_ids=SPECIALS, start_prob=0.0, seed=11 * L + 4)
    add("all", stretch_rows(R, L, 300 + L, 7), special_ids=SPECIALS, start_prob=1.0, len_lo=3, len_hi=3, seed=11 * L + 5)
    add("len1", rows, mask, None, special_ids=SPECIALS, start_prob=0.3, len_lo=1, len_hi=1, seed=11 * L + 6)
    add("long", plain, special_ids=(), start_prob=0.04, len_lo=1, len_hi=L + 5, seed=11 * L + 7)
    add("cap1", plain, special_ids=(), start_prob=0.08, len_lo=1, len_hi=3, seed=11 * L + 8, **dict(T5, max_sentinels=1))
    add("cap2", rows, mask, seg, special_ids=SPECIALS, start_prob=0.08, len_lo=1, len_hi=3, seed=11 * L + 9, **dict(T5, max_sentinels=2))
    lrows, lmask = left_padded(R, L, 400 + L)
    add("leftpad", lrows, lmask, special_ids=SPECIALS, start_prob=0.25, seed=11 * L + 10)
    prow, pseg = packed_rows(R, L, 500 + L)
    add("packed", prow, None, pseg, special_ids=[mc.SEP, PAD], start_prob=0.25, seed=11 * L + 11, eos_id=mc.SEP)
    if L > 65:                                                 # an ineligible cell at the first and at the last lane of a chunk, spans of 3 .. 5 cells around it
        erows = np.random.RandomState(600 + L).randint(1000, 30000, size=(40, L)).astype(np.int32)
        erows[0::2, 64] = mc.SEP
        erows[1::2, 63] = mc.SEP
        add("edges", erows, special_ids=SPECIALS, start_prob=0.2, len_lo=3, len_hi=5, seed=11 * L + 12)
    # truncation: the lengths exactly at, and one below, the longest row of the "mixed" case
    full = restate_denoise(rows, mask, seg, **out[0]["kw"])
    ne, nd = int(full["enc_count"].max()), int(full["dec_count"].max())
    add("fit", rows, mask, seg, enc_len=ne, dec_len=nd, **out[0]["kw"])
    if ne > 1 and nd > 1:
        add("cut", rows, mask, seg, enc_len=ne - 1, dec_len=nd - 1, **out[0]["kw"])
    return out


@functools.lru_cache(maxsize=None)
def table(L):
    """the cases of one row length with their expected results, computed once: a list of (case, want)"""
    return [(c, restate_denoise(c["rows"], c["mask"], c["seg"], **c["kw"])) for c in cases_for(L)]


def case_named(L, name):
    return next((c, w) for c, w in table(L) if c["name"].startswith(name + "/"))


# ---- what the table is there for, read off the restatement's own output.  Chunks are the 64 cells a wave takes at a time.
def coverage(Ls):
    """-> {claim: the names of the cases that show it}"""
    found = {}
    hit = lambda claim, c: found.setdefault(claim, []).append(c["name"])
    for L in Ls:
        for c, w in table(L):
            kw = spec_of(c["kw"])
            cap = kw["max_sentinels"]
            el, raw, noise, starts, length = (w[x] for x in ("eligible", "raw", "noise", "starts", "length"))
            R = len(el)
            for r, runs in enumerate(runs_of(noise)):
                for a, b in runs:
                    if a <= 63 and b >= 64:
                        hit("a run crosses the chunk edge", c)
                    if b == 63 and L > 64:
                        hit("a run ends at the chunk edge", c)
                    if a == 64 and noise[r, :63].any() and not raw[r, 63]:
                        hit("a run begins at lane 0 behind noise of the chunk before", c)
            for r in range(R):
                for lane, cell in ((0, 64), (63, 63)):
                    # an ineligible cell at that lane with a span in front of it that reaches past it, and an eligible cell behind it that is not noise
                    if cell + 1 < L and cell >= 1 and not el[r, cell] and el[r, cell + 1] and not raw[r, cell + 1] and raw[r, cell - 1]:
                        h = cell - 1
                        while h >= 0 and el[r, h]:
                            if starts[r, h] and h + length[r, h] > cell + 1:
                                hit("an ineligible cell at lane %d cuts a span" % lane, c)
                                break
                            h -= 1
                if (starts[r] & (np.arange(L) + length[r] > L)).any() and raw[r, L - 1]:
                    hit("a start reaches past the row", c)
                nruns = int(w["run"][r].max()) + 1
                if nruns > cap and cap <= 2:
                    first_over = int(np.flatnonzero(w["run"][r] == cap)[0])          # the first cell the cap turns back into a copied cell
                    if first_over < 128:
                        hit("max_sentinels %d binds in the %s chunk" % (cap, "first" if first_over < 64 else "second"), c)
            if kw["start_prob"] == 0.0 and (w["span_count"] == 0).all() and (w["dec_count"] == 1).all():
                hit("start_prob 0", c)
            if kw["start_prob"] == 1.0 and np.array_equal(raw, el) and (L < 16 or all(len(x) > 1 for x in runs_of(raw))):          # one run per stretch
                hit("start_prob 1", c)
            if kw["len_lo"] == kw["len_hi"] == 1 and starts.any():
                hit("len 1..1", c)
            if kw["len_hi"] > L and starts.any():
                hit("len_hi above L", c)
            if c["mask"] is not None and ((np.asarray(c["mask"])[:, 0] == 0) & (np.asarray(c["mask"])[:, -1] != 0)).any():
                hit("left-padded rows", c)
            if c["seg"] is not None and (np.asarray(c["seg"]).max(axis=1) > 1).any() and c["mask"] is None:
                hit("packed rows", c)
            if (~w["present"]).all(axis=1).any():
                hit("a row of padding only", c)
            if "enc_len" in c["kw"]:
                ne, nd = int(w["enc_count"].max()), int(w["dec_count"].max())
                if c["kw"]["enc_len"] == ne and c["kw"]["dec_len"] == nd and w["status"] == 0:
                    hit("enc_len / dec_len exactly at a row's length", c)
                if c["kw"]["enc_len"] == ne - 1 and c["kw"]["dec_len"] == nd - 1 and w["status"] == 1:
                    hit("enc_len / dec_len one below a row's length", c)
    return found


CLAIMS = ["a run crosses the chunk edge", "a run ends at the chunk edge", "a run begins at lane 0 behind noise of the chunk before",
          "an ineligible cell at lane 0 cuts a span", "an ineligible cell at lane 63 cuts a span", "a start reaches past the row", "start_prob 0", "start_prob 1",
          "len 1..1", "len_hi above L", "max_sentinels 1 binds in the first chunk", "max_sentinels 1 binds in the second chunk",
          "max_sentinels 2 binds in the first chunk", "max_sentinels 2 binds in the second chunk", "left-padded rows", "packed rows", "a row of padding only",
          "enc_len / dec_len exactly at a row's length", "enc_len / dec_len one below a row's length"]
