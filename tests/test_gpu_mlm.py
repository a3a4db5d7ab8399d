"""GPU: MLM masking of rows that are on the device (RowsMlmMaskBatchDevice, k_rows_mlm) and the Python calls above it, every cell of both outputs
against the restatement of mlm_cases: every group size and the chunk boundary, token and whole-word form, with and without mask and segment
plane, offset planes of the tokenizer itself, the grid-stride round, the capacity guard over canary-filled buffers, in place, shifted plane
bases, either output alone, no allocation, determinism, every refused argument, and text -> masked tensors end to end."""
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
SPECIALS = [mc.CLS, mc.SEP, mc.PAD]
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
    return None if x is None else torch.from_numpy(np.array(x, dtype=dtype, order="C")).cuda()          # (a copy: packed text is a read-only buffer)


def shifted(x, dtype, shift):
    """x on the device at `shift` elements inside a larger buffer"""
    if x is None:
        return None
    flat = np.ascontiguousarray(x, dtype=dtype).reshape(-1)
    buf = torch.zeros(flat.size + shift + 3, dtype=I32 if dtype == np.int32 else U8, device="cuda")
    buf[shift:shift + flat.size] = torch.from_numpy(flat).cuda()
    return buf[shift:shift + flat.size]


def run(hm, rows, mask=None, seg=None, S=None, E=None, special_ids=(), probs=mc.DEFAULT_PROBS, mask_id=mc.MASK, rand_range=mc.RAND_RANGE, ignore_label=-100,
        seed=0, epoch=0, nrows=None, cap=None, inplace=False, take=(True, True), shift=0):
    """one call over canary-filled outputs of cap rows + GUARD elements -> (ids, labels) as numpy [cap * L + GUARD] (None where not taken)"""
    rows = np.ascontiguousarray(rows, dtype=np.int32)
    R, L = rows.shape
    cap = R if cap is None else cap
    d = [shifted(rows, np.int32, shift), shifted(mask, np.uint8, shift), shifted(seg, np.int32, shift), shifted(S, np.int32, shift), shifted(E, np.int32, shift)]
    if inplace:
        ids = torch.full((max(cap, R) * L + GUARD,), CANARY32, dtype=I32, device="cuda")
        ids[:R * L] = d[0]
        d[0] = ids
    else:
        ids = torch.full((cap * L + GUARD + shift,), CANARY32, dtype=I32, device="cuda")[shift:] if take[0] else None
    labels = torch.full((cap * L + GUARD + shift,), CANARY32, dtype=I32, device="cuda")[shift:] if take[1] else None
    d_n = None if nrows is None else torch.tensor([nrows], dtype=torch.int64, device="cuda")
    sp = (ctypes.c_int32 * max(len(special_ids), 1))(*special_ids)
    r = bf.lib().RowsMlmMaskBatchDevice(vp(hm), ptr(d[0]), L, cap, ptr(d_n), ptr(d[1]), ptr(d[2]), ptr(d[3]), ptr(d[4]), len(special_ids), sp, *probs, mask_id,
                                        rand_range[0], rand_range[1], ignore_label, seed, epoch, ptr(ids), ptr(labels), None)
    assert r == 0, r
    torch.cuda.synchronize()
    assert bf.lib().BfLastStatus(vp(hm)) == 0
    return None if ids is None else ids.cpu().numpy(), None if labels is None else labels.cpu().numpy()


def check(hm, rows, mask=None, seg=None, S=None, E=None, nrows=None, cap=None, heads_fn=None, **kw):
    """the call against the restatement: exact below min(cap, nrows) rows, canaries from there to the end of the guard"""
    R, L = rows.shape
    cap = R if cap is None else cap
    k = min(cap, R if nrows is None else nrows)
    call_kw = {x: kw[x] for x in kw if x in ("inplace", "take", "shift")}
    spec_kw = {x: kw[x] for x in kw if x not in call_kw}
    want = mc.restate_mlm(rows[:k], None if mask is None else mask[:k], None if seg is None else seg[:k], None if S is None else S[:k], None if E is None else E[:k],
                          heads_fn=heads_fn, **spec_kw)
    assert cap <= R
    got = run(hm, rows[:cap], *[None if a is None else a[:cap] for a in (mask, seg, S, E)], nrows=nrows, cap=cap, **spec_kw, **call_kw)
    for name, g, w in (("ids", got[0], want[0]), ("labels", got[1], want[1])):
        if g is None:
            continue
        assert np.array_equal(g[:k * L], w.reshape(-1)), (name, L, R, nrows, cap)
        if not (call_kw.get("inplace") and name == "ids"):
            assert (g[k * L:] == CANARY32).all(), (name, "past the bound", L, nrows, cap)
    return want


# ---- 1. every cell against the restatement
@pytest.mark.parametrize("L", mc.TABLE_L)
def test_1_equals_the_restatement(h, L):
    n = 0
    for R in (1, 5, 257):
        rows, mask, seg = mc.random_rows(R, L, L + R)
        S, E = mc.word_planes(R, L, L + R, long_units=L > 64)                   # L = 65, 130: units across the 64-cell chunk boundary
        for planes in ((None, None), (S, E)):
            for m, s, sp in ((None, None, ()), (mask, seg, SPECIALS)):
                want = check(h, rows, m, s, *planes, special_ids=sp, probs=(0.3, 0.8, 0.1), seed=1000 * L + n, epoch=n)
                n += 1
    assert L < 4 or ((want[1] != -100).any() and (want[1] == -100).any() and (want[0] == mc.MASK).any())


@pytest.mark.parametrize("whole_word", [False, True])
@pytest.mark.parametrize("L", [2, 6, 12])
def test_1_group_sizes_the_table_leaves_out(h, L, whole_word):
    """G = 2, 8 and 16 (the table's row lengths give G = 1, 4, 32, 64): 70 rows, so the last wave is partly past the end at each of them.  The
    whole-word inputs label 2, 8 and 18 units of more than one cell"""
    rows, mask, seg, S, E = cc.table_inputs(L, 70)
    planes = (S, E) if whole_word else (None, None)
    want = check(h, rows, mask, seg, *planes, special_ids=cc.TABLE_SPECIALS, probs=cc.PROBS, seed=L + 1)
    lab = want[1].reshape(70, L) != -100
    assert lab.any() and not lab.all()
    if whole_word:
        hd = mc.heads(mc.eligible(rows, mask, seg, cc.TABLE_SPECIALS), S, E)
        assert sum(1 for r, runs in enumerate(mc.unit_runs(hd)) for a, z in runs if lab[r, a:z + 1].all()) == {2: 2, 6: 8, 12: 18}[L]


def test_1_units_across_the_chunk_boundary(h):
    """L = 130 at G = 64: units over cells 60 .. 70 (one boundary) and 40 .. 129 (both), a row that is one unit, a unit cut by an end of INT32_MAX
    in front of a start of 0; every unit is labelled whole or not at all"""
    L, R = 130, 48
    rows = (1000 + np.arange(R * L).reshape(R, L) % 20000).astype(np.int32)
    S = np.tile(10 * np.arange(L), (R, 1)).astype(np.int32); E = S + 4
    E[1:24, 60:70] = S[1:24, 61:71] - 1
    E[24:, 40:129] = S[24:, 41:130] - 1
    E[0, :-1] = S[0, 1:] - 1
    E[30:, 99] = 0x7fffffff; S[30:, 100] = 0; E[30:, 100] = S[30:, 101] - 1
    want = check(h, rows, None, None, S, E, probs=(0.5, 0.5, 0.25), seed=4)
    lab = want[1].reshape(R, L) != -100
    whole = lambda x: x.all(axis=1) | ~x.any(axis=1)
    assert whole(lab[:1]).all() and whole(lab[1:24, 60:71]).all() and whole(lab[24:30, 40:130]).all() and whole(lab[30:, 40:100]).all() and whole(lab[30:, 100:130]).all()
    assert (lab[30:, 99] != lab[30:, 100]).any() and 3 < lab[1:24, 60].sum() < 20


@pytest.mark.parametrize("L", [16, 48])
def test_1_offset_planes_of_the_tokenizer(h, L):
    """rows, mask and offset planes as encode_batch_device(..., return_offsets=True) leaves them: words of several pieces are units"""
    text, off = bf.pack_docs([s.encode() for s in SENTENCES])
    d_text, d_off = dev(text, np.uint8), dev(off, np.int64)
    rows, mask, _, r_off, st, en = bf.encode_batch_device(h, d_text, d_off, L, mc.CLS, mc.SEP, mc.PAD, return_offsets=True)
    torch.cuda.synchronize()
    rows_n, mask_n, S, E = rows.cpu().numpy(), mask.cpu().numpy(), st.cpu().numpy(), en.cpu().numpy()
    hd = mc.heads(mc.eligible(rows_n, mask_n, None, SPECIALS), S, E)
    assert sum(len(x) for x in mc.unit_runs(hd)) > 20                            # (the inputs: dozens of words of more than one piece)
    for seed in (1, 2):
        want = mc.restate_mlm(rows_n, mask_n, None, S, E, special_ids=SPECIALS, probs=(0.4, 0.8, 0.1), seed=seed)
        ids, labels = bf.rows_mlm_mask_device(h, rows, mask=mask, starts=st, ends=en, nrows=r_off[-1:], special_ids=SPECIALS, select_prob=0.4, mask_id=mc.MASK,
                                              rand_range=mc.RAND_RANGE, seed=seed)
        assert np.array_equal(ids.cpu().numpy(), want[0]) and np.array_equal(labels.cpu().numpy(), want[1])
        lab = want[1] != -100
        assert all(lab[r, a:z + 1].all() or not lab[r, a:z + 1].any() for r, runs in enumerate(mc.unit_runs(hd)) for a, z in runs)
        assert not lab[np.isin(rows_n, SPECIALS)].any() and lab.any()


def test_2_more_rows_than_one_pass_of_the_grid(h):
    """20,000 rows of 65 cells, a wave per row: more than the largest grid (8 blocks of 256 lanes per compute unit) holds, so the grid-stride
    round runs, with a last round in which some waves hold rows past the end; the row count comes from the device"""
    L, R = 65, 20000
    assert R * 64 > torch.cuda.get_device_properties(0).multi_processor_count * 8 * 256
    rnd = np.random.RandomState(65)
    rows = rnd.randint(1000, 30000, size=(R, L)).astype(np.int32)
    rows[rnd.rand(R, L) < 0.05] = mc.SEP
    real = np.where(rnd.rand(R) < 0.75, L, rnd.randint(0, L + 1, size=R))                     # three rows of four are full: cell 64 counts
    mask = (np.arange(L)[None, :] < real[:, None]).astype(np.uint8)
    length = rnd.randint(1, 5, size=(R, L)); gap = np.where(rnd.rand(R, L) < 0.8, 0, 2)      # long units: most cross cell 64
    S = (np.cumsum(length + gap, axis=1) - length).astype(np.int32); E = (S + length - 1).astype(np.int32)
    for planes in ((None, None), (S, E)):
        check(h, rows, mask, None, *planes, special_ids=[mc.SEP], probs=(0.3, 0.8, 0.1), seed=7, nrows=R - 3, heads_fn=mc.heads_array)
    hd = mc.heads_array(mc.eligible(rows, mask, None, [mc.SEP]), S, E)
    assert (hd[:, 64] < 64).sum() > 1000 and np.array_equal(hd[:50], mc.heads(mc.eligible(rows[:50], mask[:50], None, [mc.SEP]), S[:50], E[:50]))


# ---- 3. the bound: *d_nrows below, equal to and above rows_cap
@pytest.mark.parametrize("L", [5, 33, 65])
def test_3_nothing_at_or_past_the_bound_is_written(h, L):
    R = 70
    rows, mask, seg = mc.random_rows(R, L, L)
    S, E = mc.word_planes(R, L, L, long_units=True)
    for planes in ((None, None), (S, E)):
        for nrows in (0, 1, R - 1, R, R + 5, 1 << 40):
            check(h, rows, mask, seg, *planes, special_ids=SPECIALS, probs=(0.5, 0.8, 0.1), seed=3, nrows=nrows)
        check(h, rows, mask, seg, *planes, special_ids=SPECIALS, probs=(0.5, 0.8, 0.1), seed=3, nrows=R, cap=R - 7)      # the capacity below the row count
        check(h, rows, mask, seg, *planes, special_ids=SPECIALS, probs=(0.5, 0.8, 0.1), seed=3, nrows=None, cap=R - 7)


# ---- 4. pointers and workspaces
@pytest.mark.parametrize("L", [4, 33, 130])
def test_4_in_place_shifted_bases_and_single_outputs(h, L):
    R = 37
    rows, mask, seg = mc.random_rows(R, L, L + 1)
    S, E = mc.word_planes(R, L, L + 1, long_units=True)
    kw = dict(special_ids=SPECIALS, probs=(0.5, 0.8, 0.1), seed=5)
    for planes in ((None, None), (S, E)):
        check(h, rows, mask, seg, *planes, inplace=True, **kw)                    # d_ids_out == d_rows
        check(h, rows, mask, seg, *planes, inplace=True, nrows=R - 2, **kw)
        for shift in (1, 3):                                                      # every plane 4 (12) bytes off a 16-byte boundary, the mask 1 (3) bytes
            check(h, rows, mask, seg, *planes, shift=shift, **kw)
        check(h, rows, mask, seg, *planes, take=(True, False), **kw)
        check(h, rows, mask, seg, *planes, take=(False, True), **kw)
    ids, _ = run(h, rows, mask, seg, S, E, inplace=True, nrows=R - 2, **kw)       # in place, rows at or past the bound keep their ids
    assert np.array_equal(ids[(R - 2) * L:R * L], rows[R - 2:].reshape(-1)) and (ids[R * L:] == CANARY32).all()


def test_4_no_allocation_on_a_fresh_handle():
    hm = bf.load_model(bfutil.model_path(bfutil.bert_model_name()))
    try:
        rows, mask, seg = mc.random_rows(300, 64, 1)
        S, E = mc.word_planes(300, 64, 1)
        d = [dev(rows), dev(mask, np.uint8), dev(S), dev(E)]
        torch.cuda.synchronize()
        before = bf.workspace_grows()
        for planes in ((None, None), (d[2], d[3])):
            bf.rows_mlm_mask_device(hm, d[0], mask=d[1], starts=planes[0], ends=planes[1], special_ids=SPECIALS, mask_id=mc.MASK, rand_range=mc.RAND_RANGE, seed=1)
        torch.cuda.synchronize()
        assert bf.workspace_grows() == before
    finally:
        bf.free_model(hm)


# ---- 5. determinism and arguments
def test_5_same_seed_same_result_other_epoch_other_result(h):
    rows, mask, _ = mc.random_rows(64, 64, 9)
    d_rows, d_mask = dev(rows), dev(mask, np.uint8)
    kw = dict(mask=d_mask, special_ids=SPECIALS, mask_id=mc.MASK, rand_range=mc.RAND_RANGE)
    a = bf.rows_mlm_mask_device(h, d_rows, seed=77, epoch=0, **kw)
    b = bf.rows_mlm_mask_device(h, d_rows, seed=77, epoch=0, **kw)
    c = bf.rows_mlm_mask_device(h, d_rows, seed=77, epoch=1, **kw)
    e = bf.rows_mlm_mask_device(h, d_rows, seed=78, epoch=0, **kw)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert not torch.equal(a[1], c[1]) and not torch.equal(a[1], e[1]) and not torch.equal(c[1], e[1])
    assert np.array_equal(d_rows.cpu().numpy(), rows)                             # out of place: the rows are as they were
    want = mc.restate_mlm(rows, mask, special_ids=SPECIALS, seed=77, epoch=1)
    assert np.array_equal(c[0].cpu().numpy(), want[0]) and np.array_equal(c[1].cpu().numpy(), want[1])


def test_5_refused_arguments(h):
    L = bf.lib()
    t = torch.zeros(8, dtype=I32, device="cuda"); lab = torch.zeros(8, dtype=I32, device="cuda"); m = torch.ones(8, dtype=U8, device="cuda")
    sp3 = (ctypes.c_int32 * 8)(101, 102, 0)

    def call(hm=h, rows=t, row_len=8, cap=1, S=None, E=None, nspecial=3, special=sp3, probs=(0.15, 0.8, 0.1), lo=1000, hi=30522, ids=t, labels=lab):
        return L.RowsMlmMaskBatchDevice(vp(hm) if hm else None, ptr(rows), row_len, cap, None, ptr(m), None, ptr(S), ptr(E), nspecial, special, *probs, 103, lo, hi, -100,
                                        1, 0, ptr(ids), ptr(labels), None)
    nan = float("nan")
    ok = [dict(), dict(row_len=1), dict(cap=0, rows=None, ids=None, labels=None), dict(S=t, E=t), dict(nspecial=0, special=None), dict(nspecial=8), dict(ids=None),
          dict(labels=None), dict(probs=(1.0, 1.0, 0.0), lo=5, hi=5), dict(probs=(0.0, 0.0, 0.0), lo=-1, hi=-7), dict(probs=(1.0, 0.0, 1.0), lo=0, hi=1),
          dict(row_len=1 << 20, cap=0)]
    for good in ok:
        assert call(**good) == 0, good
    bad = [dict(row_len=0), dict(row_len=-1), dict(row_len=(1 << 20) + 1), dict(cap=-1), dict(rows=None), dict(ids=None, labels=None), dict(S=t), dict(E=t),
           dict(nspecial=-1), dict(nspecial=9), dict(nspecial=1, special=None), dict(probs=(-0.01, 0.8, 0.1)), dict(probs=(1.01, 0.8, 0.1)), dict(probs=(0.15, -0.5, 0.1)),
           dict(probs=(0.15, 1.5, 0.0)), dict(probs=(0.15, 0.8, -0.1)), dict(probs=(0.15, 0.0, 1.1)), dict(probs=(0.15, 0.95, 0.1)), dict(probs=(nan, 0.8, 0.1)),
           dict(probs=(0.15, nan, 0.1)), dict(probs=(0.15, 0.8, nan)), dict(lo=-1), dict(lo=5, hi=5), dict(lo=6, hi=5), dict(hm=None)]
    for b in bad:
        assert call(**b) == E_ARG, b
    torch.cuda.synchronize()


def test_5_python_call_refuses_what_the_kernel_would_misread(h):
    rows = torch.zeros((4, 8), dtype=I32, device="cuda")
    kw = dict(mask_id=mc.MASK, rand_range=mc.RAND_RANGE, seed=1)
    for bad in (dict(mask=torch.ones((4, 8), dtype=I32, device="cuda")), dict(seg=torch.ones((4, 8), dtype=torch.int64, device="cuda")),
                dict(starts=rows), dict(starts=rows, ends=torch.zeros((4, 4), dtype=I32, device="cuda")), dict(nrows=torch.tensor([4], dtype=I32, device="cuda")),
                dict(nrows=torch.tensor([4, 4], dtype=torch.int64, device="cuda")), dict(special_ids=range(9)), dict(mask=torch.ones((4, 8), dtype=U8))):
        with pytest.raises(ValueError):
            bf.rows_mlm_mask_device(h, rows, **bad, **kw)
    with pytest.raises(ValueError):
        bf.rows_mlm_mask_device(h, torch.zeros((4, 8), dtype=torch.int64, device="cuda"), **kw)
    with pytest.raises(RuntimeError):
        bf.rows_mlm_mask_device(h, rows, select_prob=1.5, **kw)


# ---- 6. text -> masked tensors
@pytest.fixture(scope="module")
def corpus():
    text, off = bf.pack_docs([s.encode() for s in SENTENCES * 3])
    return dev(text, np.uint8), dev(off, np.int64)


@pytest.mark.parametrize("whole_word", [False, True])
def test_6_encode_mlm_rows(h, corpus, whole_word):
    L = 24
    base = bf.encode_batch_device(h, *corpus, L, mc.CLS, mc.SEP, mc.PAD, return_offsets=whole_word)
    out = bf.encode_mlm_batch_device(h, *corpus, L, mc.CLS, mc.SEP, mc.PAD, mc.MASK, mc.RAND_RANGE, seed=21, epoch=2, whole_word=whole_word, select_prob=0.4)
    torch.cuda.synchronize()
    assert len(out) == len(base) + 1 and all(torch.equal(a, b) for a, b in zip(out[1:-1], base[1:]))
    rows_n, mask_n = base[0].cpu().numpy(), base[1].cpu().numpy()
    planes = (base[4].cpu().numpy(), base[5].cpu().numpy()) if whole_word else (None, None)
    want = mc.restate_mlm(rows_n, mask_n, None, *planes, special_ids=SPECIALS, probs=(0.4, 0.8, 0.1), seed=21, epoch=2)
    assert np.array_equal(out[0].cpu().numpy(), want[0]) and np.array_equal(out[-1].cpu().numpy(), want[1])
    lab = want[1] != -100
    assert lab.any() and not lab[np.isin(rows_n, SPECIALS)].any() and (want[0][lab] == mc.MASK).any()
    if whole_word:                                                                # all cells of one unit are labelled, or none
        runs = mc.unit_runs(mc.heads(mc.eligible(rows_n, mask_n, None, SPECIALS), *planes))
        assert sum(len(x) for x in runs) > 50
        assert all(lab[r, a:z + 1].all() or not lab[r, a:z + 1].any() for r, rr in enumerate(runs) for a, z in rr)


@pytest.mark.parametrize("rows_cap", [None, 64])
def test_6_encode_mlm_packed(h, corpus, rows_cap):
    L = 48
    base = bf.encode_packed_batch_device(h, *corpus, L, mc.CLS, mc.SEP, mc.PAD, rows_cap=rows_cap)
    out = bf.encode_mlm_batch_device(h, *corpus, L, mc.CLS, mc.SEP, mc.PAD, mc.MASK, mc.RAND_RANGE, seed=22, packed=True, select_prob=0.4, rows_cap=rows_cap)
    torch.cuda.synchronize()
    n = int(base[6].item())
    assert len(out) == 8 and 1 < n < len(SENTENCES) * 3 and (rows_cap is None or n <= rows_cap)
    assert all(torch.equal(a[:n] if a.dim() == 2 else a, b[:n] if b.dim() == 2 else b) for a, b in zip(out[1:3], base[1:3])) and torch.equal(out[6], base[6])
    rows_n, seg_n = base[0].cpu().numpy()[:n], base[1].cpu().numpy()[:n]
    want = mc.restate_mlm(rows_n, None, seg_n, special_ids=SPECIALS, probs=(0.4, 0.8, 0.1), seed=22)
    assert np.array_equal(out[0].cpu().numpy()[:n], want[0]) and np.array_equal(out[7].cpu().numpy()[:n], want[1])
    lab = want[1] != -100
    assert lab.any() and not lab[seg_n == 0].any() and not lab[np.isin(rows_n, SPECIALS)].any()
    assert (out[7].cpu().numpy()[n:] == -100).all()                              # rows past the count: no prediction


def test_6_packed_rows_have_no_whole_words(h, corpus):
    with pytest.raises(ValueError):
        bf.encode_mlm_batch_device(h, *corpus, 48, mc.CLS, mc.SEP, mc.PAD, mc.MASK, mc.RAND_RANGE, seed=1, whole_word=True, packed=True)
