"""GPU: the capped MLM call (RowsMlmPredictionsBatchDevice, k_rows_mlm_cap) and the Python calls above it, all five outputs against the restatement of
mlmcap_cases over canary-filled buffers with a guard behind them: every group size, the chunk boundaries, rows whose keys live in registers and
rows whose keys live in LDS, token and whole-word form, the grid-stride round, the row bound, in place, shifted bases, each output alone, no
allocation, the status word, the base call at max_pred = 0, determinism, every refused argument, and text -> capped tensors end to end."""
import ctypes

import numpy as np
import pytest
import torch

import bfutil
import blingfire_amd as bf
import mlm_cases as mc
import mlmcap_cases as cc

pytestmark = pytest.mark.gpu

CANARY32 = mc.CANARY32
E_ARG = -1
vp = ctypes.c_void_p
I32, U8 = torch.int32, torch.uint8
GUARD = 64
SPECIALS = cc.TABLE_SPECIALS
NAMES = ("ids", "labels", "cells", "pred_labels", "count")
ALL5 = (True,) * 5
SENTENCES = ["The tokenization of unaffable embeddings is straightforward.", "Hello, world! This is a test.", "playing replayed unplayable players",
             "Sergei Alonichau saw a girl with a telescope.", "don't U.S.A. e-mail 3,000.50", "a", "", "supercalifragilisticexpialidocious",
             "Whole-word masking keeps the pieces of a word together, whatever the tokenizer made of it.", "internationalization and localization",
             "x" * 40 + " " + "y" * 9, "The quick brown fox jumps over the lazy dog near the riverbank at dawn", "antidisestablishmentarianism!",
             "pretraining pretrained pretrains", "café naïve coöperate", "[CLS] [SEP] [MASK] literal brackets", "one two three four five six seven eight nine ten",
             "unbelievably unmistakable unforgettable", "GPU kernels; wavefronts, shuffles & scans.", "tokenizers' offsets (inclusive ends) matter",
             "rereading misreading proofreading", "  leading and trailing spaces  ", "hyphen-ated words-and-more", "numbers 1234567890 0987654321",
             "ALLCAPS MixedCase lowercase", "counterintuitively overgeneralized", "a b c d e f g h i j k l m n o p q r s t u v w x y z", "end."]


@pytest.fixture(scope="module")
def h():
    hm = bf.load_model(bfutil.model_path(bfutil.bert_model_name()))
    yield hm
    bf.free_model(hm)


def ptr(t):
    return None if t is None else t if isinstance(t, int) else t.data_ptr()


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


def call(hm, d, L, cap, d_n, special_ids, probs, mask_id, rand_range, ignore_label, seed, epoch, outs, P, entry=None):
    sp = (ctypes.c_int32 * max(len(special_ids), 1))(*special_ids)
    head = (vp(hm), ptr(d[0]), L, cap, ptr(d_n), ptr(d[1]), ptr(d[2]), ptr(d[3]), ptr(d[4]), len(special_ids), sp, *probs, mask_id, rand_range[0], rand_range[1],
            ignore_label, seed, epoch, ptr(outs[0]), ptr(outs[1]))
    if entry == "base":
        return bf.lib().RowsMlmMaskBatchDevice(*head, None)
    return bf.lib().RowsMlmPredictionsBatchDevice(*head, P, ptr(outs[2]), ptr(outs[3]), ptr(outs[4]), None)


def run(hm, rows, mask=None, seg=None, S=None, E=None, special_ids=(), probs=mc.DEFAULT_PROBS, mask_id=mc.MASK, rand_range=mc.RAND_RANGE, ignore_label=-100,
        seed=0, epoch=0, nrows=None, cap=None, max_pred=1, inplace=False, take=ALL5, shift=0, entry=None):
    """one call over canary-filled outputs of cap rows + GUARD elements -> the five outputs as flat numpy arrays (None where not taken)"""
    rows = np.ascontiguousarray(rows, dtype=np.int32)
    R, L = rows.shape
    cap = R if cap is None else cap
    P = max_pred
    d = [shifted(rows, np.int32, shift), shifted(mask, np.uint8, shift), shifted(seg, np.int32, shift), shifted(S, np.int32, shift), shifted(E, np.int32, shift)]
    outs = [canary(n, shift) if t else None for n, t in zip((cap * L, cap * L, cap * P, cap * P, cap), take)]
    if P == 0:
        outs[2:] = [None, None, None]
    if inplace:
        outs[0] = torch.full((max(cap, R) * L + GUARD,), CANARY32, dtype=I32, device="cuda")
        outs[0][:R * L] = d[0]
        d[0] = outs[0]
    d_n = None if nrows is None else torch.tensor([nrows], dtype=torch.int64, device="cuda")
    r = call(hm, d, L, cap, d_n, special_ids, probs, mask_id, rand_range, ignore_label, seed, epoch, outs, P, entry)
    assert r == 0, r
    torch.cuda.synchronize()
    assert bf.lib().BfLastStatus(vp(hm)) == 0
    return [None if o is None else o.cpu().numpy() for o in outs]


def check(hm, rows, mask=None, seg=None, S=None, E=None, nrows=None, cap=None, heads_fn=None, kept_fn=None, **kw):
    """the call against the restatement: exact below min(cap, nrows) rows, canaries from there to the end of the guard, in all five outputs"""
    R, L = rows.shape
    cap = R if cap is None else cap
    k = min(cap, R if nrows is None else nrows)
    call_kw = {x: kw[x] for x in kw if x in ("inplace", "take", "shift")}
    spec_kw = {x: kw[x] for x in kw if x not in call_kw}
    P = spec_kw["max_pred"]
    want = cc.restate_cap(rows[:k], *[None if a is None else a[:k] for a in (mask, seg, S, E)], heads_fn=heads_fn, kept_fn=kept_fn, **spec_kw)
    assert cap <= R
    got = run(hm, rows[:cap], *[None if a is None else a[:cap] for a in (mask, seg, S, E)], nrows=nrows, cap=cap, **spec_kw, **call_kw)
    for name, g, w, width in zip(NAMES, got, want, (L, L, P, P, 1)):
        if g is None:
            continue
        assert np.array_equal(g[:k * width], w.reshape(-1)), (name, L, R, nrows, cap, P)
        if not (call_kw.get("inplace") and name == "ids"):
            assert (g[k * width:] == CANARY32).all(), (name, "past the bound", L, nrows, cap, P)
    return want


# ---- 1. every cell against the restatement
@pytest.mark.parametrize("L", mc.TABLE_L)
def test_1_equals_the_restatement(h, L):
    n = 0
    for R in (1, 5, 257):
        rows, mask, seg, S, E = cc.table_inputs(L, R)
        for planes in ((None, None), (S, E)):
            for m, s, sp in ((None, None, ()), (mask, seg, SPECIALS)):
                for P in cc.table_P(L):
                    check(h, rows, m, s, *planes, special_ids=sp, probs=cc.PROBS, seed=7 if sp else 1000 * L + n, epoch=0 if sp else n, max_pred=P,
                          heads_fn=mc.heads_array, kept_fn=cc.kept_array)
                    n += 1
            if R == 257 and L >= 31:                                              # the inputs: both branches of the kernel, in a quarter of the rows each at least
                binds, free, _ = cc.shares(rows, mask, seg, *planes, max(1, L // 8), special_ids=SPECIALS, probs=cc.PROBS, seed=7)
                assert binds >= 0.25 and free >= 0.25, (L, binds, free)
        if R == 257 and L >= 31:
            assert min(cc.shares(rows, mask, seg, S, E, P, special_ids=SPECIALS, probs=cc.PROBS, seed=7)[2] for P in (1, 2)) >= 0.04


@pytest.mark.parametrize("whole_word", [False, True])
@pytest.mark.parametrize("L", [2, 6, 12])
def test_1_group_sizes_the_table_leaves_out(h, L, whole_word):
    """G = 2, 8 and 16 (the table's row lengths give G = 1, 4, 32, 64): 70 rows, so the last wave is partly past the end at each of them; at P = 1
    the cap binds in some rows and leaves others with their selection whole"""
    rows, mask, seg, S, E = cc.table_inputs(L, 70)
    planes = (S, E) if whole_word else (None, None)
    check(h, rows, mask, seg, *planes, special_ids=SPECIALS, probs=cc.PROBS, seed=L + 1, max_pred=1)
    binds, free, _ = cc.shares(rows, mask, seg, *planes, 1, special_ids=SPECIALS, probs=cc.PROBS, seed=L + 1)
    assert binds > 0 and free > 0, (L, binds, free)


# ---- 2. chunk boundaries
def test_2_units_across_the_chunk_boundaries(h):
    """L = 130 at G = 64 (three chunks, keys in registers): units over cells 60 .. 70 and 40 .. 129, a row that is one unit.  P = 5 is smaller than
    those units, P = 95 holds the long one; kept cells of the second and third chunk land in the right gather slots"""
    L, R = 130, 48
    rows = (1000 + np.arange(R * L).reshape(R, L) % 20000).astype(np.int32)
    S = np.tile(10 * np.arange(L), (R, 1)).astype(np.int32); E = S + 4
    E[1:24, 60:70] = S[1:24, 61:71] - 1
    E[24:, 40:129] = S[24:, 41:130] - 1
    E[0, :-1] = S[0, 1:] - 1
    both = False
    for P in (5, 95):
        want = check(h, rows, None, None, S, E, probs=(0.5, 0.5, 0.25), seed=4, max_pred=P)
        lab = want[1] != -100
        whole = lambda x: x.all(axis=1) | ~x.any(axis=1)
        assert whole(lab[:1]).all() and whole(lab[1:24, 60:71]).all() and whole(lab[24:, 40:130]).all() and not lab[0].any()
        assert not lab[1:24, 60:71].any() if P == 5 else lab[1:24, 60:71].any()
        assert not lab[24:, 40:130].any() if P == 5 else lab[24:, 40:130].any()
        both = both or bool((lab[:, :64].any(axis=1) & lab[:, 64:].any(axis=1)).any())
        assert (want[4] > 0).any()
    assert both                                                                   # some row keeps cells on both sides of cell 64


# ---- 3. the long-row storage (keys in LDS beyond 256 cells)
@pytest.mark.parametrize("L", [513, 2048, 4096])
def test_3_long_rows(h, L):
    R = 3
    rnd = np.random.RandomState(L)
    rows = rnd.randint(1000, 30000, size=(R, L)).astype(np.int32)
    length = rnd.randint(1, 5, size=(R, L)); gap = np.where(rnd.rand(R, L) < 0.6, 0, 2)
    S = (np.cumsum(length + gap, axis=1) - length).astype(np.int32); E = (S + length - 1).astype(np.int32)
    for planes in ((None, None), (S, E)):
        for select in (1.0, 0.15):
            for P in (1, 600, L):
                check(h, rows, None, None, *planes, probs=(select, 0.8, 0.1), seed=L, max_pred=P, heads_fn=mc.heads_array, kept_fn=cc.kept_array)


def test_3_rows_longer_than_the_cap_supports(h):
    L = cc.MAX_LEN + 1
    rows = np.random.RandomState(1).randint(1000, 30000, size=(2, L)).astype(np.int32)
    d = [dev(rows), None, None, None, None]
    outs = [canary(2 * L), canary(2 * L), canary(2), canary(2), canary(2)]
    args = ((), mc.DEFAULT_PROBS, mc.MASK, mc.RAND_RANGE, -100, 5, 0)
    assert call(h, d, L, 2, None, *args, outs, 1) == E_ARG
    got = run(h, rows, seed=5, max_pred=0)                                        # P = 0: the base call, any length
    want = mc.restate_mlm(rows, seed=5, heads_fn=mc.heads_array)
    assert np.array_equal(got[0][:2 * L], want[0].reshape(-1)) and np.array_equal(got[1][:2 * L], want[1].reshape(-1))
    torch.cuda.synchronize()
    assert all((o.cpu().numpy() == CANARY32).all() for o in outs)


# ---- 4. more rows than one pass of the grid
def test_4_more_rows_than_one_pass_of_the_grid(h):
    L, R = 65, 20000
    assert R * 64 > torch.cuda.get_device_properties(0).multi_processor_count * 8 * 256
    rnd = np.random.RandomState(65)
    rows = rnd.randint(1000, 30000, size=(R, L)).astype(np.int32)
    rows[rnd.rand(R, L) < 0.05] = mc.SEP
    real = np.where(rnd.rand(R) < 0.75, L, rnd.randint(0, L + 1, size=R))
    mask = (np.arange(L)[None, :] < real[:, None]).astype(np.uint8)
    length = rnd.randint(1, 5, size=(R, L)); gap = np.where(rnd.rand(R, L) < 0.8, 0, 2)
    S = (np.cumsum(length + gap, axis=1) - length).astype(np.int32); E = (S + length - 1).astype(np.int32)
    for planes in ((None, None), (S, E)):
        want = check(h, rows, mask, None, *planes, special_ids=[mc.SEP], probs=cc.PROBS, seed=7, nrows=R - 3, max_pred=8, heads_fn=mc.heads_array, kept_fn=cc.kept_array)
        assert (want[4][:R - 3] == 8).mean() > 0.1 and (want[4][:R - 3] < 8).mean() > 0.1          # (the inputs: rows the cap binds in exactly, and rows below it)
    small = cc.restate_cap(rows[:40], mask[:40], None, S[:40], E[:40], special_ids=[mc.SEP], probs=cc.PROBS, seed=7, max_pred=8)
    assert all(np.array_equal(a, b[:40]) for a, b in zip(small, want))            # (the array form of the restatement against its loop, on these rows)


# ---- 5. the bound
@pytest.mark.parametrize("L", [5, 33, 65])
def test_5_nothing_at_or_past_the_bound_is_written(h, L):
    R = 70
    rows, mask, seg = mc.random_rows(R, L, L)
    S, E = mc.word_planes(R, L, L, long_units=True)
    kw = dict(special_ids=SPECIALS, probs=(0.5, 0.8, 0.1), seed=3, max_pred=max(2, L // 8), heads_fn=mc.heads_array, kept_fn=cc.kept_array)
    for planes in ((None, None), (S, E)):
        for nrows in (0, 1, R - 1, R, R + 5, 1 << 40):
            check(h, rows, mask, seg, *planes, nrows=nrows, **kw)
        check(h, rows, mask, seg, *planes, nrows=R, cap=R - 7, **kw)
        check(h, rows, mask, seg, *planes, nrows=None, cap=R - 7, **kw)


# ---- 6. pointers and outputs
@pytest.mark.parametrize("L", [4, 33, 130])
def test_6_in_place_shifted_bases_and_single_outputs(h, L):
    R = 37
    rows, mask, seg = mc.random_rows(R, L, L + 1)
    S, E = mc.word_planes(R, L, L + 1, long_units=True)
    kw = dict(special_ids=SPECIALS, probs=(0.5, 1.0, 0.0), seed=5, max_pred=max(2, L // 4))
    for planes in ((None, None), (S, E)):
        want = check(h, rows, mask, seg, *planes, inplace=True, **kw)             # d_ids_out == d_rows
        k = want[4] > 0
        assert k.any()                                                            # every kept cell became mask_id; the gathered labels are the ids that were there
        for r in np.flatnonzero(k):
            c = want[2][r, :want[4][r]]
            assert (want[0][r, c] == mc.MASK).all() and np.array_equal(want[3][r, :want[4][r]], rows[r, c]) and (rows[r, c] != mc.MASK).all()
        check(h, rows, mask, seg, *planes, inplace=True, nrows=R - 2, **kw)
        for shift in (1, 3):
            check(h, rows, mask, seg, *planes, shift=shift, **kw)
        for i in range(5):
            check(h, rows, mask, seg, *planes, take=tuple(j == i for j in range(5)), **kw)
    got = run(h, rows, mask, seg, S, E, inplace=True, nrows=R - 2, **kw)          # in place, rows at or past the bound keep their ids
    assert np.array_equal(got[0][(R - 2) * L:R * L], rows[R - 2:].reshape(-1)) and (got[0][R * L:] == CANARY32).all()


def test_6_no_allocation_on_a_fresh_handle():
    hm = bf.load_model(bfutil.model_path(bfutil.bert_model_name()))
    try:
        d = {}
        for L in (64, 130, 600):
            rows, mask, _ = mc.random_rows(300, L, 1)
            S, E = mc.word_planes(300, L, 1)
            d[L] = [dev(rows), dev(mask, np.uint8), dev(S), dev(E)]
        torch.cuda.synchronize()
        before = bf.workspace_grows()
        for L, t in d.items():
            for planes in ((None, None), (t[2], t[3])):
                bf.rows_mlm_mask_device(hm, t[0], mask=t[1], starts=planes[0], ends=planes[1], special_ids=SPECIALS, mask_id=mc.MASK, rand_range=mc.RAND_RANGE, seed=1,
                                        max_predictions=L // 8)
        torch.cuda.synchronize()
        assert bf.workspace_grows() == before
    finally:
        bf.free_model(hm)


def test_6_the_status_word_is_cleared(h):
    """a row call whose rows_cap is too small leaves bit 0 set; the capped call behind it clears the word and sets nothing"""
    ids = torch.arange(1000, 1040, dtype=I32, device="cuda")
    off = torch.tensor([0, 40], dtype=torch.int64, device="cuda")
    L = 8
    out = [torch.zeros(L, dtype=I32, device="cuda"), torch.zeros(L, dtype=U8, device="cuda"), torch.zeros(1, dtype=I32, device="cuda"),
           torch.zeros(1, dtype=I32, device="cuda"), torch.zeros(2, dtype=torch.int64, device="cuda")]
    lib = bf.lib()
    r = lib.IdsToRowsBatchDevice(vp(h), ptr(ids), 40, ptr(off), 1, L, mc.CLS, mc.SEP, mc.PAD, 4, 100, 0, ptr(out[0]), ptr(out[1]), ptr(out[2]), ptr(out[3]), 1,
                                 ptr(out[4]), None)          # 40 ids in windows of 6: ten rows, room for one
    torch.cuda.synchronize()
    assert r == 0 and lib.BfLastStatus(vp(h)) & 1
    rows, mask, _ = mc.random_rows(9, 33, 2)
    check(h, rows, mask, special_ids=SPECIALS, probs=cc.PROBS, seed=1, max_pred=3)          # (run() asserts a status of 0)


# ---- 7. the base call
@pytest.mark.parametrize("L", [33, 130, 600])
def test_7_max_pred_0_is_the_base_call(h, L):
    R = 50
    rows, mask, seg = mc.random_rows(R, L, L + 2)
    S, E = mc.word_planes(R, L, L + 2, long_units=True)
    kw = dict(special_ids=SPECIALS, probs=cc.PROBS, seed=8, epoch=2, nrows=R - 1)
    for planes in ((None, None), (S, E)):
        base = run(h, rows, mask, seg, *planes, max_pred=0, entry="base", **kw)
        zero = run(h, rows, mask, seg, *planes, max_pred=0, **kw)
        assert np.array_equal(base[0], zero[0]) and np.array_equal(base[1], zero[1])          # byte for byte, canaries and guard included
        full = run(h, rows, mask, seg, *planes, max_pred=L, **kw)
        assert np.array_equal(base[0], full[0]) and np.array_equal(base[1], full[1])
        want = mc.restate_mlm(rows[:R - 1], mask[:R - 1], seg[:R - 1], *[None if a is None else a[:R - 1] for a in planes], special_ids=SPECIALS, probs=cc.PROBS,
                              seed=8, epoch=2, heads_fn=mc.heads_array)
        assert np.array_equal(base[1][:(R - 1) * L], want[1].reshape(-1)) and np.array_equal(full[4][:R - 1], (want[1] != -100).sum(axis=1))


# ---- 8. determinism
def test_8_same_call_same_result(h):
    rows, mask, _ = mc.random_rows(64, 64, 9)
    d_rows, d_mask = dev(rows), dev(mask, np.uint8)
    kw = dict(mask=d_mask, special_ids=SPECIALS, mask_id=mc.MASK, rand_range=mc.RAND_RANGE, select_prob=0.3, max_predictions=8)
    a = bf.rows_mlm_mask_device(h, d_rows, seed=77, epoch=0, **kw)
    b = bf.rows_mlm_mask_device(h, d_rows, seed=77, epoch=0, **kw)
    c = bf.rows_mlm_mask_device(h, d_rows, seed=77, epoch=1, **kw)
    e = bf.rows_mlm_mask_device(h, d_rows, seed=78, epoch=0, **kw)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert not torch.equal(a[2], c[2]) and not torch.equal(a[2], e[2]) and not torch.equal(c[1], e[1])
    assert np.array_equal(d_rows.cpu().numpy(), rows)
    big = torch.zeros((100, 64), dtype=I32, device="cuda"); big[:64] = d_rows     # a larger rows_cap, the same d_nrows: the same rows
    bmask = torch.ones((100, 64), dtype=U8, device="cuda"); bmask[:64] = d_mask
    n = torch.tensor([64], dtype=torch.int64, device="cuda")
    f = bf.rows_mlm_mask_device(h, big, seed=77, epoch=0, nrows=n, **dict(kw, mask=bmask))
    assert all(torch.equal(x[:64], y) for x, y in zip(f, a)) and int(f[4][64:].sum()) == 0 and bool((f[3][64:] == -100).all())


# ---- 9. refused arguments
def test_9_refused_arguments(h):
    L = bf.lib()
    t = torch.zeros(8, dtype=I32, device="cuda"); lab = torch.zeros(8, dtype=I32, device="cuda"); m = torch.ones(8, dtype=U8, device="cuda")
    g = [torch.zeros(16, dtype=I32, device="cuda") for _ in range(3)]
    sp3 = (ctypes.c_int32 * 8)(101, 102, 0)

    def call9(hm=h, rows=t, row_len=8, cap=1, S=None, E=None, nspecial=3, special=sp3, probs=(0.15, 0.8, 0.1), lo=1000, hi=30522, ids=t, labels=lab, P=4,
              cells=g[0], pl=g[1], cnt=g[2]):
        return L.RowsMlmPredictionsBatchDevice(vp(hm) if hm else None, ptr(rows), row_len, cap, None, ptr(m), None, ptr(S), ptr(E), nspecial, special, *probs, 103, lo, hi,
                                               -100, 1, 0, ptr(ids), ptr(labels), P, ptr(cells), ptr(pl), ptr(cnt), None)
    nan = float("nan")
    none3 = dict(cells=None, pl=None, cnt=None)
    ok = [dict(), dict(row_len=1), dict(cap=0, rows=None, ids=None, labels=None, **none3), dict(P=1 << 20, cap=0), dict(P=9), dict(P=8), dict(S=t, E=t),
          dict(nspecial=0, special=None), dict(ids=None, labels=None), dict(ids=None, labels=None, cells=None, pl=None), dict(**none3), dict(P=0, **none3),
          dict(P=0, row_len=1 << 20, cap=0, **none3), dict(row_len=4096, cap=0), dict(probs=(1.0, 1.0, 0.0), lo=5, hi=5)]
    for good in ok:
        assert call9(**good) == 0, good
    bad = [dict(row_len=0), dict(row_len=-1), dict(row_len=(1 << 20) + 1, P=0, **none3), dict(cap=-1), dict(rows=None), dict(ids=None, labels=None, **none3), dict(S=t),
           dict(E=t), dict(nspecial=-1), dict(nspecial=9), dict(nspecial=1, special=None), dict(probs=(-0.01, 0.8, 0.1)), dict(probs=(1.01, 0.8, 0.1)),
           dict(probs=(0.15, 0.95, 0.1)), dict(probs=(nan, 0.8, 0.1)), dict(probs=(0.15, 0.8, nan)), dict(lo=-1), dict(lo=5, hi=5), dict(hm=None),
           dict(P=-1), dict(P=(1 << 20) + 1), dict(P=(1 << 20) + 1, cap=0), dict(row_len=4097, cap=0), dict(row_len=1 << 20, cap=0),
           dict(P=0), dict(P=0, cells=None, pl=None), dict(P=0, pl=None, cnt=None), dict(P=0, cells=None, cnt=None), dict(P=0, ids=None, labels=None, **none3)]
    for b in bad:
        assert call9(**b) == E_ARG, b
    torch.cuda.synchronize()


# ---- 10. Python
@pytest.fixture(scope="module")
def corpus():
    text, off = bf.pack_docs([s.encode() for s in SENTENCES * 3])
    return dev(text, np.uint8), dev(off, np.int64)


def gathers(labels, cells, plabels, count, ignore=-100):
    labels, cells, plabels, count = [x.cpu().numpy() for x in (labels, cells, plabels, count)]
    assert np.array_equal(count, (labels != ignore).sum(axis=1))
    for r in range(len(labels)):
        k = int(count[r])
        assert np.array_equal(labels[r, cells[r, :k]], plabels[r, :k]) and (cells[r, k:] == 0).all() and (plabels[r, k:] == ignore).all()


def test_10_rows_mlm_mask_device(h):
    rows, mask, seg = mc.random_rows(40, 48, 3)
    d_rows, d_mask = dev(rows), dev(mask, np.uint8)
    kw = dict(mask=d_mask, special_ids=SPECIALS, mask_id=mc.MASK, rand_range=mc.RAND_RANGE, select_prob=0.3, seed=4)
    out = bf.rows_mlm_mask_device(h, d_rows, max_predictions=6, **kw)
    torch.cuda.synchronize()
    assert len(out) == 5 and out[2].shape == (40, 6) and out[3].shape == (40, 6) and out[4].shape == (40,) and all(o.dtype == I32 for o in out)
    want = cc.restate_cap(rows, mask, special_ids=SPECIALS, probs=cc.PROBS, seed=4, max_pred=6)
    assert all(np.array_equal(o.cpu().numpy(), w) for o, w in zip(out, want))
    gathers(*out[1:])
    assert len(bf.rows_mlm_mask_device(h, d_rows, **kw)) == 2 and len(bf.rows_mlm_mask_device(h, d_rows, max_predictions=0, **kw)) == 2
    for bad in (-1, 2.0, "3", None, True):
        with pytest.raises(ValueError):
            bf.rows_mlm_mask_device(h, d_rows, max_predictions=bad, **kw)
    long_rows = torch.zeros((1, 4097), dtype=I32, device="cuda")
    with pytest.raises(ValueError):
        bf.rows_mlm_mask_device(h, long_rows, mask_id=mc.MASK, rand_range=mc.RAND_RANGE, seed=1, max_predictions=5)
    assert len(bf.rows_mlm_mask_device(h, long_rows, mask_id=mc.MASK, rand_range=mc.RAND_RANGE, seed=1)) == 2


@pytest.mark.parametrize("whole_word", [False, True])
def test_10_encode_mlm_rows(h, corpus, whole_word):
    L, P = 24, 4
    base = bf.encode_batch_device(h, *corpus, L, mc.CLS, mc.SEP, mc.PAD, return_offsets=whole_word)
    out = bf.encode_mlm_batch_device(h, *corpus, L, mc.CLS, mc.SEP, mc.PAD, mc.MASK, mc.RAND_RANGE, seed=21, epoch=2, whole_word=whole_word, select_prob=0.4,
                                     max_predictions=P)
    torch.cuda.synchronize()
    assert len(out) == len(base) + 4 and all(torch.equal(a, b) for a, b in zip(out[1:-4], base[1:]))
    rows_n, mask_n = base[0].cpu().numpy(), base[1].cpu().numpy()
    planes = (base[4].cpu().numpy(), base[5].cpu().numpy()) if whole_word else (None, None)
    want = cc.restate_cap(rows_n, mask_n, None, *planes, special_ids=SPECIALS, probs=(0.4, 0.8, 0.1), seed=21, epoch=2, max_pred=P)
    assert all(np.array_equal(o.cpu().numpy(), w) for o, w in zip((out[0],) + tuple(out[-4:]), want))
    gathers(*out[-4:])
    lab = want[1] != -100
    uncapped = mc.restate_mlm(rows_n, mask_n, None, *planes, special_ids=SPECIALS, probs=(0.4, 0.8, 0.1), seed=21, epoch=2)[1] != -100
    assert lab.any() and (uncapped.sum(axis=1) > lab.sum(axis=1)).any() and (want[4] <= P).all()          # some row is capped
    if whole_word:
        runs = mc.unit_runs(mc.heads(mc.eligible(rows_n, mask_n, None, SPECIALS), *planes))
        assert all(lab[r, a:z + 1].all() or not lab[r, a:z + 1].any() for r, rr in enumerate(runs) for a, z in rr)


def test_10_encode_mlm_packed(h, corpus):
    L, P = 48, 6
    base = bf.encode_packed_batch_device(h, *corpus, L, mc.CLS, mc.SEP, mc.PAD, rows_cap=64)
    out = bf.encode_mlm_batch_device(h, *corpus, L, mc.CLS, mc.SEP, mc.PAD, mc.MASK, mc.RAND_RANGE, seed=22, packed=True, select_prob=0.4, rows_cap=64, max_predictions=P)
    torch.cuda.synchronize()
    n = int(base[6].item())
    assert len(out) == 11 and 1 < n < 64
    rows_n, seg_n = base[0].cpu().numpy()[:n], base[1].cpu().numpy()[:n]
    want = cc.restate_cap(rows_n, None, seg_n, special_ids=SPECIALS, probs=(0.4, 0.8, 0.1), seed=22, max_pred=P)
    assert all(np.array_equal(o.cpu().numpy()[:n], w) for o, w in zip((out[0],) + tuple(out[7:]), want))
    gathers(*out[7:])
    assert (out[7].cpu().numpy()[n:] == -100).all() and (out[8].cpu().numpy()[n:] == 0).all() and (out[9].cpu().numpy()[n:] == -100).all()
    assert (out[10].cpu().numpy()[n:] == 0).all() and (want[4] == P).any()        # rows past the count hold no predictions
