"""CPU tier of the MLM masking call (RowsMlmMaskBatchDevice): the known answers of Philox4x32-10 pin the generator of the restatement
(mlm_cases) and of the lane code; the lane code of blingfire_amd/csrc/bf_mlm.h, compiled for the host and driven in the kernel's lane partition
with G lanes, chunks and the carry (tests/hosttest/bf_mlmtest.cpp), is held to the restatement cell by cell; the restatement itself is held to
the shares its probabilities promise; and the new symbol is declared and exported."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import bfutil
import mlm_cases as mc

c_i64, c_int, c_vp, c_dbl = ctypes.c_int64, ctypes.c_int, ctypes.c_void_p, ctypes.c_double
GROUPS = [1, 2, 4, 8, 16, 32, 64]
HOST_L = mc.TABLE_L + [200]
SPECIALS8 = [mc.CLS, mc.SEP, mc.PAD, 5, 6, 7, 8, 9]


@pytest.fixture(scope="module")
def ht():
    L = ctypes.CDLL(bfutil.HOSTTEST_LIB)
    L.bft_philox.restype = None
    L.bft_philox.argtypes = [c_vp, c_vp, c_vp]
    L.bft_mlm_thresholds.restype = c_int
    L.bft_mlm_thresholds.argtypes = [c_dbl, c_dbl, c_dbl, c_int, c_int, c_vp]
    L.bft_mlm_rows.restype = c_int
    L.bft_mlm_rows.argtypes = [c_vp, c_int, c_i64, c_i64, c_vp, c_vp, c_vp, c_vp, c_int, c_vp, c_dbl, c_dbl, c_dbl, c_int, c_int, c_int, c_int, ctypes.c_uint64,
                               ctypes.c_uint32, c_vp, c_vp, c_int]
    return L


def host_mlm(ht, rows, mask=None, seg=None, S=None, E=None, special_ids=(), probs=mc.DEFAULT_PROBS, mask_id=mc.MASK, rand_range=mc.RAND_RANGE, ignore_label=-100,
             seed=0, epoch=0, row_base=0, group=0, inplace=False):
    rows = np.ascontiguousarray(rows, dtype=np.int32)
    R, L = rows.shape
    arr = [None if a is None else np.ascontiguousarray(a, dtype=t) for a, t in ((mask, np.uint8), (seg, np.int32), (S, np.int32), (E, np.int32))]
    ids = rows.copy() if inplace else np.full((R, L), mc.CANARY32, dtype=np.int32)
    labels = np.full((R, L), mc.CANARY32, dtype=np.int32)
    sp = (ctypes.c_int32 * max(len(special_ids), 1))(*special_ids)
    r = ht.bft_mlm_rows((ids if inplace else rows).ctypes.data, L, R, row_base, *[None if a is None else a.ctypes.data for a in arr], len(special_ids), sp, *probs,
                        mask_id, rand_range[0], rand_range[1], ignore_label, seed, epoch, ids.ctypes.data, labels.ctypes.data, group)
    assert r == 0
    return ids, labels


def same(got, want):
    return np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


# ---- (a) the generator
def test_a_philox_known_answers(ht):
    for c, k, want in mc.PHILOX_VECTORS:
        assert tuple(int(x) for x in mc.philox(*c, *k)) == want
        cc, kk, out = (ctypes.c_uint32 * 4)(*c), (ctypes.c_uint32 * 2)(*k), (ctypes.c_uint32 * 4)()
        ht.bft_philox(cc, kk, out)
        assert tuple(out) == want


def test_a_philox_over_arrays_equals_scalars():
    rnd = np.random.RandomState(1)
    c = rnd.randint(0, 2 ** 32, size=(6, 50), dtype=np.uint64)
    got = mc.philox(*c)
    for i in (0, 17, 49):
        assert tuple(int(x[i]) for x in got) == tuple(int(x) for x in mc.philox(*[int(v) for v in c[:, i]]))


def test_a_row_indices_above_2_to_32(ht):
    """hi32(r) is in the counter: rows 2^32 apart draw differently, and the lane code agrees with the restatement there"""
    rows, mask, _ = mc.random_rows(6, 33, 5)
    S, E = mc.word_planes(6, 33, 5)
    outs = []
    for base in (0, 1 << 32, (1 << 32) + 3, (5 << 32) + 1, (1 << 40) + 7):
        for planes in ((None, None), (S, E)):
            want = mc.restate_mlm(rows, mask, None, *planes, special_ids=[mc.PAD], probs=(0.5, 0.8, 0.1), seed=9, row_base=base)
            assert same(host_mlm(ht, rows, mask, None, *planes, special_ids=[mc.PAD], probs=(0.5, 0.8, 0.1), seed=9, row_base=base), want), base
        outs.append(want[1])
    assert not np.array_equal(outs[0], outs[1]) and not np.array_equal(outs[1], outs[3])
    a = mc.draw(np.array([7, 7 + (1 << 32)]), np.array([3, 3]), 1, 0)
    assert int(a[0][0]) != int(a[0][1])


def test_a_thresholds(ht):
    out = (ctypes.c_uint64 * 3)()
    for probs in ((0.15, 0.8, 0.1), (1.0, 1.0, 0.0), (0.0, 0.0, 0.0), (1.0, 0.0, 1.0), (0.3, 1e-12, 0.999), (0.1 + 0.2, 0.7, 0.3)):
        assert ht.bft_mlm_thresholds(*probs, 0, 1, out) == 0
        ts, tm, tr = mc.thresholds(*probs)
        assert tuple(out) == (ts, tm, tm + tr), probs
    assert mc.thresholds(1.0, 0.5, 0.0)[0] == 1 << 32
    nan = float("nan")
    for bad in ((-0.1, 0.8, 0.1), (1.1, 0.8, 0.1), (0.15, 0.95, 0.1), (nan, 0.8, 0.1), (0.15, nan, 0.1), (0.15, 0.8, nan), (0.15, -1e-9, 0.1), (0.15, 0.8, 1.5)):
        assert ht.bft_mlm_thresholds(*bad, 0, 1, out) == -1, bad
    # a random share needs a range; none needs none
    assert ht.bft_mlm_thresholds(0.15, 0.8, 0.1, 5, 5, out) == -1 and ht.bft_mlm_thresholds(0.15, 0.8, 0.1, -1, 5, out) == -1
    assert ht.bft_mlm_thresholds(0.15, 0.8, 0.0, 5, 5, out) == 0


# ---- (b) the lane code against the restatement
@pytest.mark.parametrize("L", HOST_L)
def test_b_every_group_size_equals_the_restatement(ht, L):
    R = 7
    rows, mask, seg = mc.random_rows(R, L, L)
    n = 0
    for long_units in (False, True):
        S, E = mc.word_planes(R, L, L, long_units)
        for planes in ((None, None), (S, E)):
            for m, s, sp in ((None, None, ()), (mask, None, [mc.CLS, mc.SEP, mc.PAD]), (None, seg, SPECIALS8), (mask, seg, [mc.PAD])):
                kw = dict(special_ids=sp, probs=(0.3, 0.8, 0.1), seed=L * 1000 + n, epoch=n)
                want = mc.restate_mlm(rows, m, s, *planes, **kw)
                for G in GROUPS + [0]:
                    assert same(host_mlm(ht, rows, m, s, *planes, group=G, **kw), want), (L, G, n)
                assert same(host_mlm(ht, rows, m, s, *planes, inplace=True, **kw), want)
                n += 1
    assert L < 4 or ((want[1] != -100).any() and (want[1] == -100).any())


def test_b_units_across_chunk_boundaries(ht):
    """L = 200 at G = 64: units over one boundary (cells 60 .. 70), over two (100 .. 195: the chunks at 128 and 192), a row that is one unit; the
    head of every cell is the unit's first cell, so the whole unit is labelled or none of it"""
    L, R = 200, 40
    rows = (1000 + np.arange(R * L).reshape(R, L) % 20000).astype(np.int32)
    S = np.tile(10 * np.arange(L), (R, 1)).astype(np.int32); E = S + 4          # gaps everywhere ...
    for a, z in ((60, 70), (100, 195)):                                        # ... but inside these runs
        E[1:, a:z] = S[1:, a + 1:z + 1] - 1
    E[0, :-1] = S[0, 1:] - 1                                                    # row 0: one unit
    el = np.ones((R, L), dtype=bool)
    h = mc.heads(el, S, E)
    assert (h[0] == 0).all() and (h[1, 60:71] == 60).all() and (h[1, 100:196] == 100).all() and h[1, 71] == 71 and h[1, 196] == 196
    want = mc.restate_mlm(rows, None, None, S, E, probs=(0.5, 0.5, 0.25), seed=4)
    for G in GROUPS + [0]:
        assert same(host_mlm(ht, rows, None, None, S, E, probs=(0.5, 0.5, 0.25), seed=4, group=G), want), G
    lab = want[1] != -100
    for r in range(1, R):
        assert lab[r, 60:71].all() or not lab[r, 60:71].any()
        assert lab[r, 100:196].all() or not lab[r, 100:196].any()
    assert lab[0].all() or not lab[0].any()
    assert 5 < lab[1:, 100].sum() < R - 5 and len({bool(x) for x in lab[:, 0]}) == 2          # (the inputs: both outcomes occur)
    ids = want[0][1:, 100:196][lab[1:, 100]]                                    # the pieces of a selected unit take their own actions
    assert (ids == mc.MASK).any() and (ids != mc.MASK).any()


def test_b_what_breaks_a_unit(ht):
    """an ineligible cell (mask, segment, special), a negative start on either side, and an end of INT32_MAX in front of a start of 0 (E + 1
    would wrap to the start; S - 1 does not) each end the unit"""
    L = 12
    rows = (2000 + np.arange(L)[None, :]).astype(np.int32).copy()
    S = (3 * np.arange(L)[None, :]).astype(np.int32); E = S + 2                 # byte-adjacent from end to end
    mask = np.ones((1, L), dtype=np.uint8); seg = np.ones((1, L), dtype=np.int32)
    assert (mc.heads(np.ones((1, L), dtype=bool), S, E) == 0).all()
    rows[0, 2] = mc.SEP; mask[0, 4] = 0; seg[0, 6] = 0
    S[0, 8] = -1
    S2, E2 = S.copy(), E.copy()
    E2[0, 9] = 0x7fffffff; S2[0, 10] = 0; E2[0, 10] = S2[0, 11] - 1
    el = mc.eligible(rows, mask, seg, [mc.SEP])
    assert mc.heads(el, S, E)[0].tolist() == [0, 0, 2, 3, 4, 5, 6, 7, 8, 9, 9, 9]
    assert mc.heads(el, S2, E2)[0].tolist() == [0, 0, 2, 3, 4, 5, 6, 7, 8, 9, 10, 10]
    many = np.tile(rows, (64, 1))                                               # 64 rows: every outcome of the draws occurs
    for s, e in ((S, E), (S2, E2)):
        kw = dict(special_ids=[mc.SEP], probs=(0.5, 1.0, 0.0), seed=11)
        want = mc.restate_mlm(many, np.tile(mask, (64, 1)), np.tile(seg, (64, 1)), np.tile(s, (64, 1)), np.tile(e, (64, 1)), **kw)
        for G in (0, 1, 4, 64):
            assert same(host_mlm(ht, many, np.tile(mask, (64, 1)), np.tile(seg, (64, 1)), np.tile(s, (64, 1)), np.tile(e, (64, 1)), group=G, **kw), want), G
        lab = want[1] != -100
        assert not lab[:, [2, 4, 6]].any() and (lab[:, 0] == lab[:, 1]).all() and (lab[:, 7] != lab[:, 8]).any() and (lab[:, 8] != lab[:, 9]).any()
    assert (lab[:, 9] != lab[:, 10]).any() and (lab[:, 10] == lab[:, 11]).all()


@pytest.mark.parametrize("probs", [(0.0, 0.8, 0.1), (1.0, 1.0, 0.0), (1.0, 0.0, 1.0), (1.0, 0.0, 0.0), (1.0, 0.5, 0.5)])
def test_b_probabilities_0_and_1(ht, probs):
    rows, mask, seg = mc.random_rows(9, 65, 3)
    S, E = mc.word_planes(9, 65, 3)
    for planes in ((None, None), (S, E)):
        want = mc.restate_mlm(rows, mask, seg, *planes, special_ids=[mc.CLS, mc.SEP, mc.PAD], probs=probs, seed=2)
        assert same(host_mlm(ht, rows, mask, seg, *planes, special_ids=[mc.CLS, mc.SEP, mc.PAD], probs=probs, seed=2), want)
        el = mc.eligible(rows, mask, seg, [mc.CLS, mc.SEP, mc.PAD])
        ids, labels = want
        assert ((labels != -100) == (el if probs[0] == 1.0 else np.zeros_like(el))).all() and (ids[~el] == rows[~el]).all()
        if probs == (1.0, 1.0, 0.0):
            assert (ids[el] == mc.MASK).all()
        if probs == (1.0, 0.0, 1.0):
            assert ((ids[el] >= mc.RAND_RANGE[0]) & (ids[el] < mc.RAND_RANGE[1])).all() and (ids[el] != rows[el]).any()
        if probs == (1.0, 0.0, 0.0) or probs[0] == 0.0:
            assert np.array_equal(ids, rows)
        if probs == (1.0, 0.5, 0.5):
            assert ((ids[el] == mc.MASK) | ((ids[el] >= mc.RAND_RANGE[0]) & (ids[el] < mc.RAND_RANGE[1]))).all() and 0.4 < (ids[el] == mc.MASK).mean() < 0.6


def test_b_nspecial_0_and_8(ht):
    rows, _, _ = mc.random_rows(5, 64, 8, specials=SPECIALS8)
    for sp in ((), SPECIALS8):
        want = mc.restate_mlm(rows, special_ids=sp, probs=(1.0, 1.0, 0.0), seed=1)
        assert same(host_mlm(ht, rows, special_ids=sp, probs=(1.0, 1.0, 0.0), seed=1), want)
        hit = np.isin(rows, SPECIALS8)
        assert hit.any() and ((want[1][hit] == -100).all() if sp else (want[1] != -100).all())


def test_b_seed_and_epoch_matter(ht):
    rows, _, _ = mc.random_rows(8, 64, 2, specials=())
    base = host_mlm(ht, rows, seed=5, epoch=0)
    assert same(base, host_mlm(ht, rows, seed=5, epoch=0))
    for kw in (dict(seed=6, epoch=0), dict(seed=5, epoch=1), dict(seed=5 + (1 << 32), epoch=0)):
        other = host_mlm(ht, rows, **kw)
        assert same(other, mc.restate_mlm(rows, **kw)) and not np.array_equal(other[1], base[1]), kw


def test_b_array_form_of_the_heads_equals_the_loop():
    for L, seed in ((1, 1), (7, 2), (65, 3), (200, 4)):
        rows, mask, seg = mc.random_rows(12, L, seed)
        el = mc.eligible(rows, mask, seg, [mc.CLS])
        for long_units in (False, True):
            S, E = mc.word_planes(12, L, seed, long_units)
            if L > 2:
                E[3, 0] = 0x7fffffff; S[3, 1] = 0; S[5, 1] = -(2 ** 31)
            assert np.array_equal(mc.heads(el, S, E), mc.heads_array(el, S, E)), L
        assert np.array_equal(mc.heads(el, None, None), mc.heads_array(el, None, None))


# ---- (c) the restatement itself: the shares its probabilities promise
@pytest.mark.parametrize("seed", [1, 12345, 0])
def test_c_shares_of_the_restatement(seed):
    """65,536 eligible cells (1024 rows of 64) at 0.15 / 0.8 / 0.1: the selected share within 0.15 +- 0.01 (seeds 1, 12345 and 0 give 0.1499,
    0.1490 and 0.1526 in this arrangement), the mask and random shares of the selected cells within +- 0.02 of 0.8 and 0.1; random ids inside
    [1000, 30522)"""
    rows = np.full((1024, 64), 7, dtype=np.int32)
    ids, labels = mc.restate_mlm(rows, seed=seed)
    sel = labels != -100
    assert (labels[sel] == 7).all() and (ids[~sel] == 7).all()
    print("seed %d: selected %.4f, mask %.4f, random %.4f" % (seed, sel.mean(), (ids[sel] == mc.MASK).mean(), ((ids[sel] != mc.MASK) & (ids[sel] != 7)).mean()))
    assert abs(sel.mean() - 0.15) <= 0.01
    masked = ids[sel] == mc.MASK
    rand = ~masked & (ids[sel] != 7)
    assert abs(masked.mean() - 0.8) <= 0.02 and abs(rand.mean() - 0.1) <= 0.02
    r = ids[sel][rand]
    assert r.min() >= 1000 and r.max() < 30522


# ---- (d) declared and exported; the stand-alone program
def test_d_new_symbol_is_declared_and_exported():
    import blingfire_amd as bf
    hdr = open(os.path.join(bfutil.ROOT, "include", "blingfiretokdll_amd.h")).read()
    exports = open(os.path.join(bfutil.ROOT, "blingfire_amd", "csrc", "exports.map")).read()
    lib = ctypes.CDLL(bf.LIB_PATH)
    name = "RowsMlmMaskBatchDevice"
    assert re.search(r"BF_API\s+\w+\s+%s\(" % name, hdr)
    assert re.search(r"^\s*%s;" % name, exports, flags=re.M)
    assert hasattr(lib, name)
    assert re.search(r"#define\s+BF_MLM_MAX_SPECIAL\s+8\b", hdr)
    assert os.path.exists(os.path.join(bfutil.ROOT, "blingfire_amd", "csrc", "bf_mlm.h"))
    assert callable(bf.rows_mlm_mask_device) and callable(bf.encode_mlm_batch_device)


def test_stand_alone_program_under_sanitizers(tmp_path):
    """the lane-code driver with its own main, built with -fsanitize=address,undefined and run as a program (never loaded into python)"""
    exe = str(tmp_path / "bf_mlmtest")
    src = os.path.join(bfutil.ROOT, "tests", "hosttest", "bf_mlmtest.cpp")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-DBF_MLMTEST_MAIN", src, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("mlm ok:"), r.stdout + r.stderr
