"""GPU: the span-corruption call (RowsDenoiseBatchDevice, k_rows_denoise) and the Python calls above it, all seven outputs and the status word
against the restatement of denoise_cases over canary-filled buffers with a guard behind them: every case of the table (every group size, the
chunk edges, the cap, the truncated forms), the grid-stride round, the row bound, shifted bases, each output alone, independence of the grid,
the status word, no allocation, every refused argument, and text -> encoder and decoder rows end to end from stream rows and from rows."""
import ctypes

import numpy as np
import pytest
import torch

import bfutil
import blingfire_amd as bf
import denoise_cases as dc
import mlm_cases as mc
from test_gpu_mlmcap import SENTENCES

pytestmark = pytest.mark.gpu

CANARY32 = dc.CANARY32
E_ARG = -1
vp = ctypes.c_void_p
I32, U8 = torch.int32, torch.uint8
GUARD = 64
ALL7 = (True,) * 7


@pytest.fixture(scope="module")
def h():
    hm = bf.load_model(bfutil.model_path(bfutil.bert_model_name()))
    yield hm
    bf.free_model(hm)


def ptr(t):
    return None if t is None else t.data_ptr()


def dev(x, dtype=np.int32):
    return None if x is None else torch.from_numpy(np.array(x, dtype=dtype, order="C")).cuda()


def shifted(x, dtype, shift):
    """x on the device at `shift` elements inside a larger buffer"""
    if x is None:
        return None
    flat = np.ascontiguousarray(x, dtype=dtype).reshape(-1)
    buf = torch.zeros(flat.size + shift + 3, dtype=I32 if dtype == np.int32 else U8, device="cuda")
    buf[shift:shift + flat.size] = torch.from_numpy(flat).cuda()
    return buf[shift:shift + flat.size]


def canary(n, shift=0):
    return torch.full((n + GUARD + shift,), CANARY32, dtype=I32, device="cuda")[shift:]


def widths(EL, DL):
    return dict(enc=EL, enc_cell=EL, enc_count=1, dec=DL, dec_cell=DL, dec_count=1, span_count=1)


def call(hm, d_rows, L, cap, d_n, d_mask, d_seg, s, EL, DL, outs):
    sp = (ctypes.c_int32 * max(len(s["special_ids"]), 1))(*s["special_ids"])
    return bf.lib().RowsDenoiseBatchDevice(vp(hm), ptr(d_rows), L, cap, ptr(d_n), ptr(d_mask), ptr(d_seg), len(s["special_ids"]), sp, s["start_prob"], s["len_lo"], s["len_hi"],
                                           s["sentinel_first"], s["sentinel_step"], s["max_sentinels"], -1 if s["eos_id"] is None else s["eos_id"], s["pad_id"],
                                           s["ignore_label"], s["seed"], s["epoch"], EL, ptr(outs["enc"]), ptr(outs["enc_cell"]), ptr(outs["enc_count"]), DL, ptr(outs["dec"]),
                                           ptr(outs["dec_cell"]), ptr(outs["dec_count"]), ptr(outs["span_count"]), None)


def run(hm, rows, mask=None, seg=None, nrows=None, cap=None, enc_len=None, dec_len=None, take=ALL7, shift=0, **kw):
    """one call over canary-filled outputs of cap rows + GUARD elements -> the seven outputs as flat numpy arrays (None where not taken) and `status`"""
    rows = np.ascontiguousarray(rows, dtype=np.int32)
    R, L = rows.shape
    cap = R if cap is None else cap
    EL = L if enc_len is None else enc_len
    DL = L + 2 if dec_len is None else dec_len
    w = widths(EL, DL)
    outs = {n: canary(cap * w[n], shift) if t else None for n, t in zip(dc.NAMES, take)}
    d_n = None if nrows is None else torch.tensor([nrows], dtype=torch.int64, device="cuda")
    r = call(hm, shifted(rows, np.int32, shift), L, cap, d_n, shifted(mask, np.uint8, shift), shifted(seg, np.int32, shift), dc.spec_of(kw), EL, DL, outs)
    assert r == 0, r
    torch.cuda.synchronize()
    got = {n: None if o is None else o.cpu().numpy() for n, o in outs.items()}
    got["status"] = bf.lib().BfLastStatus(vp(hm))
    return got


def check(hm, rows, mask=None, seg=None, nrows=None, cap=None, want=None, array=False, status=None, **kw):
    """the call against the restatement: exact below min(cap, nrows) rows, canaries from there to the end of the guard, in all seven outputs"""
    R, L = rows.shape
    cap = R if cap is None else cap
    assert cap <= R
    k = min(cap, R if nrows is None else nrows)
    call_kw = {x: kw[x] for x in kw if x in ("take", "shift")}
    spec_kw = {x: kw[x] for x in kw if x not in call_kw}
    cut = lambda a, n: None if a is None else a[:n]
    if want is None:
        want = dc.restate_denoise(rows[:k], cut(mask, k), cut(seg, k), array=array, **spec_kw)
    got = run(hm, rows[:cap], cut(mask, cap), cut(seg, cap), nrows=nrows, cap=cap, **spec_kw, **call_kw)
    w = widths(L if spec_kw.get("enc_len") is None else spec_kw["enc_len"], L + 2 if spec_kw.get("dec_len") is None else spec_kw["dec_len"])
    for name in dc.NAMES:
        g = got[name]
        if g is None:
            continue
        assert np.array_equal(g[:k * w[name]], want[name][:k].reshape(-1)), (name, L, R, nrows, cap)
        assert (g[k * w[name]:] == CANARY32).all(), (name, "past the bound", L, nrows, cap)
    side = lambda a, b: call_kw.get("take", ALL7)[a] or call_kw.get("take", ALL7)[b]
    if status is None:                                        # bit 0 only for a side the caller takes
        status = 1 if (side(0, 1) and (want["enc_count"][:k] > w["enc"]).any()) or (side(3, 4) and (want["dec_count"][:k] > w["dec"]).any()) else 0
    assert got["status"] == status, (got["status"], status)
    return want


# ---- 1. every case of the table
@pytest.mark.parametrize("L", dc.TABLE_L)
def test_1_equals_the_restatement(h, L):
    for c, want in dc.table(L):
        check(h, c["rows"], c["mask"], c["seg"], want=want, status=want["status"], **c["kw"])


def test_1_the_table_contains_its_claims():
    found = dc.coverage(dc.TABLE_L)
    assert all(found.get(claim) for claim in dc.CLAIMS), [c for c in dc.CLAIMS if not found.get(c)]


# ---- 2. more rows than one pass of the grid, the row count from the device
def test_2_more_rows_than_one_pass_of_the_grid(h):
    """20,000 rows of 65 cells, a wave per row: more than the largest grid (8 blocks of 256 lanes per compute unit) holds, so the grid-stride
    round runs, with a last round in which some waves hold rows past the end"""
    L, R = 65, 20000
    assert R * 64 > torch.cuda.get_device_properties(0).multi_processor_count * 8 * 256
    rnd = np.random.RandomState(65)
    rows = rnd.randint(1000, 30000, size=(R, L)).astype(np.int32)
    rows[rnd.rand(R, L) < 0.05] = mc.SEP
    real = np.where(rnd.rand(R) < 0.75, L, rnd.randint(0, L + 1, size=R))
    mask = (np.arange(L)[None, :] < real[:, None]).astype(np.uint8)
    kw = dict(special_ids=[mc.SEP], start_prob=0.1, seed=7)
    want = check(h, rows, mask, nrows=R - 3, array=True, **kw)
    assert (want["noise"][:, 63] & want["noise"][:, 64]).mean() > 0.05                       # (the inputs: runs over the chunk edge in a twentieth of the rows)
    small = dc.restate_denoise(rows[:40], mask[:40], **kw)
    assert all(np.array_equal(small[n], want[n][:40]) for n in dc.NAMES)                    # (the array form of the restatement against its loop, on these rows)


# ---- 3. the bound
@pytest.mark.parametrize("L", [5, 33, 65])
def test_3_nothing_at_or_past_the_bound_is_written(h, L):
    R = 70
    rows, mask, seg = mc.random_rows(R, L, L)
    kw = dict(special_ids=dc.SPECIALS, start_prob=0.3, seed=3, array=True)
    for nrows in (0, 1, R - 1, R, R + 5, 1 << 40):
        check(h, rows, mask, seg, nrows=nrows, **kw)
    check(h, rows, mask, seg, nrows=R, cap=R - 7, **kw)
    check(h, rows, mask, seg, nrows=None, cap=R - 7, **kw)


# ---- 4. pointers and outputs
@pytest.mark.parametrize("L", [4, 33, 129])
def test_4_shifted_bases_and_single_outputs(h, L):
    c, want = dc.case_named(L, "mixed")
    for shift in (1, 3):                                      # every pointer at its natural alignment only (the mask at any byte)
        check(h, c["rows"], c["mask"], c["seg"], want=want, shift=shift, **c["kw"])
    for i in range(7):
        check(h, c["rows"], c["mask"], c["seg"], want=want, take=tuple(j == i for j in range(7)), **c["kw"])
    c, want = dc.case_named(L, "cut")                          # a side that is not taken loses nothing: only the side taken sets the bit
    for take in ((True, False, False, False, False, False, False), (False, False, False, False, True, False, False), (False, False, True, False, False, True, True)):
        check(h, c["rows"], c["mask"], c["seg"], want=want, take=take, **c["kw"])
    got = run(h, c["rows"], c["mask"], c["seg"], take=(False, False, True, False, False, True, True), **dict(c["kw"], enc_len=-7, dec_len=0))
    assert got["status"] == 0 and np.array_equal(got["dec_count"][:len(c["rows"])], want["dec_count"])          # counts alone: the lengths are not looked at


def test_4_the_result_does_not_depend_on_the_grid(h):
    rows, mask, seg = mc.random_rows(64, 65, 9)
    kw = dict(special_ids=dc.SPECIALS, start_prob=0.25, seed=77)
    a = run(h, rows, mask, seg, **kw)
    big_rows = np.zeros((20000, 65), dtype=np.int32); big_rows[:64] = rows
    big_mask = np.ones((20000, 65), dtype=np.uint8); big_mask[:64] = mask
    big_seg = np.ones((20000, 65), dtype=np.int32); big_seg[:64] = seg
    b = run(h, big_rows, big_mask, big_seg, nrows=64, **kw)   # a larger rows_cap and grid, the same d_nrows: the same rows
    w = widths(65, 67)
    for n in dc.NAMES:
        assert np.array_equal(a[n][:64 * w[n]], b[n][:64 * w[n]]) and (b[n][64 * w[n]:] == CANARY32).all(), n
    e = run(h, rows, mask, seg, **dict(kw, epoch=1))
    assert not np.array_equal(a["dec"], e["dec"]) and a["status"] == b["status"] == 0


# ---- 5. the status word, no allocation
def test_5_truncation_sets_bit_0_and_a_clean_call_clears_it(h):
    c, want = dc.case_named(65, "cut")
    assert want["status"] == 1
    check(h, c["rows"], c["mask"], c["seg"], want=want, status=1, **c["kw"])
    c, want = dc.case_named(65, "fit")
    check(h, c["rows"], c["mask"], c["seg"], want=want, status=0, **c["kw"])                # (the word is the call's own)


def test_5_no_allocation_on_a_fresh_handle():
    hm = bf.load_model(bfutil.model_path(bfutil.bert_model_name()))
    try:
        d = {}
        for L in (16, 64, 130, 600):
            rows, mask, _ = mc.random_rows(300, L, 1)
            d[L] = [dev(rows), dev(mask, np.uint8)]
        torch.cuda.synchronize()
        before = bf.workspace_grows()
        for L, t in d.items():
            bf.rows_denoise_device(hm, t[0], mask=t[1], special_ids=dc.SPECIALS, start_prob=0.05, sentinel_first=32099, eos_id=dc.EOS, seed=1, return_cells=True)
        torch.cuda.synchronize()
        assert bf.workspace_grows() == before
    finally:
        bf.free_model(hm)


# ---- 6. refused arguments
def test_6_refused_arguments(h):
    L = bf.lib()
    t = torch.zeros(16, dtype=I32, device="cuda")
    o = [torch.zeros(32, dtype=I32, device="cuda") for _ in range(7)]
    sp3 = (ctypes.c_int32 * 8)(1, 0, 102)
    all7 = dict(enc=o[0], ecell=o[1], ecnt=o[2], dec=o[3], dcell=o[4], dcnt=o[5], spans=o[6])
    none7 = {k: None for k in all7}

    def call6(hm=h, rows=t, row_len=8, cap=2, nspecial=3, special=sp3, prob=0.15, lo=1, hi=5, first=32099, step=-1, ms=100, enc_len=8, dec_len=10, **outs):
        q = dict(all7, **outs)
        return L.RowsDenoiseBatchDevice(vp(hm) if hm else None, ptr(rows), row_len, cap, None, None, None, nspecial, special, prob, lo, hi, first, step, ms, 1, 0, -100, 1, 0,
                                        enc_len, ptr(q["enc"]), ptr(q["ecell"]), ptr(q["ecnt"]), dec_len, ptr(q["dec"]), ptr(q["dcell"]), ptr(q["dcnt"]), ptr(q["spans"]), None)
    nan = float("nan")
    ok = [dict(), dict(row_len=1, enc_len=1, dec_len=3), dict(cap=0, rows=None, **none7), dict(row_len=1 << 20, enc_len=1 << 20, dec_len=1 << 20, cap=0),
          dict(nspecial=0, special=None), dict(prob=0.0), dict(prob=1.0), dict(lo=1 << 20, hi=1 << 20), dict(ms=1, first=0), dict(ms=1 << 20, first=0, step=1, cap=0),
          dict(first=(1 << 31) - 100, step=1), dict(first=99), dict(enc_len=0, enc=None, ecell=None), dict(dec_len=-3, dec=None, dcell=None),
          dict(**dict(none7, spans=o[6])), dict(enc_len=1, dec_len=1)]
    for good in ok:
        assert call6(**good) == 0, good
    bad = [dict(row_len=0), dict(row_len=-1), dict(row_len=(1 << 20) + 1, cap=0), dict(cap=-1), dict(rows=None), dict(**none7), dict(enc_len=0), dict(enc_len=(1 << 20) + 1),
           dict(dec_len=0), dict(dec_len=(1 << 20) + 1), dict(enc_len=0, enc=None), dict(dec_len=0, dcell=None), dict(nspecial=-1), dict(nspecial=9),
           dict(nspecial=1, special=None), dict(prob=-0.01), dict(prob=1.01), dict(prob=nan), dict(lo=0), dict(lo=6, hi=5), dict(hi=(1 << 20) + 1), dict(ms=0),
           dict(ms=(1 << 20) + 1), dict(first=-1), dict(first=98), dict(first=(1 << 31) - 99, step=1), dict(hm=None)]
    for b in bad:
        assert call6(**b) == E_ARG, b
    torch.cuda.synchronize()


# ---- 7. Python
@pytest.fixture(scope="module")
def corpus():
    text, off = bf.pack_docs([s.encode() for s in SENTENCES * 3])
    return dev(text, np.uint8), dev(off, np.int64)


def test_7_rows_denoise_device(h):
    c, want = dc.case_named(33, "mixed")
    kw = dc.spec_of(c["kw"])
    out = bf.rows_denoise_device(h, dev(c["rows"]), mask=dev(c["mask"], np.uint8), seg=dev(c["seg"]), return_cells=True, **kw)
    torch.cuda.synchronize()
    names = dict(input_ids="enc", labels="dec", enc_count="enc_count", dec_count="dec_count", span_count="span_count", enc_cells="enc_cell", dec_cells="dec_cell")
    assert set(out) == set(names) and out["input_ids"].shape == (12, 33) and out["labels"].shape == (12, 35) and all(t.dtype == I32 for t in out.values())
    assert all(np.array_equal(out[k].cpu().numpy(), want[n]) for k, n in names.items())
    # the cell planes carry another plane of the input into the new layout with one gather
    seg_enc = dev(c["seg"]).gather(1, out["enc_cells"].clamp(min=0).long()).cpu().numpy()
    at = want["enc_cell"] >= 0
    assert np.array_equal(seg_enc[at], np.take_along_axis(c["seg"], np.maximum(want["enc_cell"], 0), axis=1)[at])
    assert set(bf.rows_denoise_device(h, dev(c["rows"]), **kw)) == set(names) - {"enc_cells", "dec_cells"}
    n = torch.tensor([5], dtype=torch.int64, device="cuda")   # rows at or past nrows: padding, ignore_label, counts of 0
    part = bf.rows_denoise_device(h, dev(c["rows"]), mask=dev(c["mask"], np.uint8), seg=dev(c["seg"]), nrows=n, **kw)
    assert np.array_equal(part["labels"].cpu().numpy()[:5], want["dec"][:5]) and bool((part["labels"][5:] == -100).all()) and int(part["dec_count"][5:].sum()) == 0
    with pytest.raises(ValueError):
        bf.rows_denoise_device(h, dev(c["rows"]).long(), **kw)
    with pytest.raises(RuntimeError):
        bf.rows_denoise_device(h, dev(c["rows"]), **dict(kw, start_prob=1.5))


@pytest.mark.parametrize("source", ["stream", "rows"])
def test_7_encode_denoise_end_to_end(h, corpus, source):
    """the BERT model with made-up sentinel ids (the last ids of its vocabulary, downwards) and [SEP] as the eos"""
    L = 24
    spec = dict(sentinel_first=30521, sentinel_step=-1, max_sentinels=100, start_prob=0.2, len_lo=1, len_hi=4, seed=31, epoch=2)
    out = bf.encode_denoise_batch_device(h, *corpus, L, mc.SEP, mc.PAD, spec["sentinel_first"], spec["seed"], epoch=2, source=source, start_prob=0.2, len_hi=4,
                                         return_cells=True)
    torch.cuda.synchronize()
    assert bf.lib().BfLastStatus(vp(h)) == 0
    if source == "stream":
        base = bf.encode_clm_batch_device(h, *corpus, L, None, mc.SEP, mc.PAD)
        rows, seg, mask, n = base["input_ids"].cpu().numpy(), base["seg"].cpu().numpy(), None, int(base["nrows"][0].item())
        assert np.array_equal(out["seg"].cpu().numpy()[:n], seg[:n])
    else:
        base = bf.encode_batch_device(h, *corpus, L, None, mc.SEP, mc.PAD)
        rows, mask, seg, n = base[0].cpu().numpy(), base[1].cpu().numpy(), None, int(base[3][-1].item())
        assert np.array_equal(out["mask"].cpu().numpy()[:n], mask[:n])
    assert n > 1 and int(out["nrows"].item()) == n and np.array_equal(out["rows"].cpu().numpy()[:n], rows[:n])
    want = dc.restate_denoise(rows[:n], None if mask is None else mask[:n], None if seg is None else seg[:n], special_ids=sorted({mc.SEP, mc.PAD}), eos_id=mc.SEP,
                              pad_id=mc.PAD, **spec)
    names = dict(input_ids="enc", labels="dec", enc_count="enc_count", dec_count="dec_count", span_count="span_count", enc_cells="enc_cell", dec_cells="dec_cell")
    for k, name in names.items():
        assert np.array_equal(out[k].cpu().numpy()[:n], want[name]), (k, source)
    assert (want["span_count"] > 0).any() and (out["labels"].cpu().numpy()[n:] == -100).all()
