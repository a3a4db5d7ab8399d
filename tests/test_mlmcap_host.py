"""CPU tier of the capped MLM call (RowsMlmPredictionsBatchDevice): the lane code of blingfire_amd/csrc/bf_mlm.h (key, compare, threshold search,
"kept", gather slot with its carry), compiled for the host and driven in the kernel's partition (tests/hosttest/bf_mlmcaptest.cpp), is held to
the restatement of mlmcap_cases in all five outputs; the search is held to hand-made keys; the restatement's array form is held to its loop; the
table inputs are shown to exercise both branches; the rule keeps units whole and prefers no position; and the symbol is declared and exported."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import bfutil
import mlm_cases as mc
import mlmcap_cases as cc

c_i64, c_int, c_vp, c_dbl = ctypes.c_int64, ctypes.c_int, ctypes.c_void_p, ctypes.c_double
GROUPS = [1, 2, 4, 8, 16, 32, 64]
HOST_L = mc.TABLE_L + [200]
NONE = (1 << 64) - 1
NAMES = ("ids", "labels", "cells", "pred_labels", "count")


@pytest.fixture(scope="module")
def ht():
    L = ctypes.CDLL(bfutil.HOSTTEST_LIB)
    L.bft_mlmcap_rows.restype = c_int
    L.bft_mlmcap_rows.argtypes = [c_vp, c_int, c_i64, c_i64, c_vp, c_vp, c_vp, c_vp, c_int, c_vp, c_dbl, c_dbl, c_dbl, c_int, c_int, c_int, c_int, ctypes.c_uint64,
                                  ctypes.c_uint32, c_vp, c_vp, c_int, c_vp, c_vp, c_vp, c_int]
    L.bft_mlmcap_search.restype = c_int
    L.bft_mlmcap_search.argtypes = [c_vp, c_int, c_int, c_int, c_vp, c_vp]
    L.bft_mlmcap_key.restype = ctypes.c_uint64
    L.bft_mlmcap_key.argtypes = [ctypes.c_uint32, c_int]
    return L


def host_cap(ht, rows, mask=None, seg=None, S=None, E=None, special_ids=(), probs=mc.DEFAULT_PROBS, mask_id=mc.MASK, rand_range=mc.RAND_RANGE, ignore_label=-100,
             seed=0, epoch=0, row_base=0, max_pred=1, group=0, inplace=False):
    rows = np.ascontiguousarray(rows, dtype=np.int32)
    R, L = rows.shape
    arr = [None if a is None else np.ascontiguousarray(a, dtype=t) for a, t in ((mask, np.uint8), (seg, np.int32), (S, np.int32), (E, np.int32))]
    ids = rows.copy() if inplace else np.full((R, L), mc.CANARY32, dtype=np.int32)
    labels = np.full((R, L), mc.CANARY32, dtype=np.int32)
    cells = np.full((R, max_pred), mc.CANARY32, dtype=np.int32); plabels = np.full((R, max_pred), mc.CANARY32, dtype=np.int32)
    count = np.full((R,), mc.CANARY32, dtype=np.int32)
    sp = (ctypes.c_int32 * max(len(special_ids), 1))(*special_ids)
    r = ht.bft_mlmcap_rows((ids if inplace else rows).ctypes.data, L, R, row_base, *[None if a is None else a.ctypes.data for a in arr], len(special_ids), sp, *probs,
                           mask_id, rand_range[0], rand_range[1], ignore_label, seed, epoch, ids.ctypes.data, labels.ctypes.data, max_pred, cells.ctypes.data,
                           plabels.ctypes.data, count.ctypes.data, group)
    assert r == 0
    return ids, labels, cells, plabels, count


def same(got, want, what=None):
    for name, g, w in zip(NAMES, got, want):
        assert np.array_equal(g, w), (name, what)
    return True


def search(ht, words, P, G):
    w = (ctypes.c_uint64 * len(words))(*words)
    kept = np.zeros(len(words), dtype=np.uint8); slot = np.zeros(len(words), dtype=np.int32)
    n = ht.bft_mlmcap_search(w, len(words), G, P, kept.ctypes.data, slot.ctypes.data)
    assert n == int(kept.sum()) and slot[kept != 0].tolist() == list(range(n)) and (slot[kept == 0] == -1).all()
    return kept.astype(bool).tolist()


def key(w3, h):
    return (w3 << 32) | h


# ---- (a) the lane code against the restatement
@pytest.mark.parametrize("L", HOST_L)
def test_a_every_group_size_equals_the_restatement(ht, L):
    R = 7
    rows, mask, seg = mc.random_rows(R, L, L)
    n = 0
    for long_units in (False, True):
        S, E = mc.word_planes(R, L, L, long_units)
        for planes in ((None, None), (S, E)):
            if long_units and planes[0] is None:
                continue                                                          # (the token form has no units: once is enough)
            for m, s, sp in ((None, None, ()), (mask, seg, cc.TABLE_SPECIALS)):
                for P in cc.table_P(L):
                    kw = dict(special_ids=sp, probs=cc.PROBS, seed=L * 1000 + n, epoch=n, max_pred=P)
                    want = cc.restate_cap(rows, m, s, *planes, **kw)
                    for G in GROUPS + [0]:
                        same(host_cap(ht, rows, m, s, *planes, group=G, **kw), want, (L, G, P, n))
                    same(host_cap(ht, rows, m, s, *planes, inplace=True, **kw), want, (L, "in place", P, n))
                    n += 1


def test_a_row_indices_above_2_to_32(ht):
    rows, mask, _ = mc.random_rows(6, 33, 5)
    S, E = mc.word_planes(6, 33, 5)
    for base in (0, (1 << 32) + 3, (1 << 40) + 7):
        for planes in ((None, None), (S, E)):
            kw = dict(special_ids=[mc.PAD], probs=(0.5, 0.8, 0.1), seed=9, row_base=base, max_pred=4)
            same(host_cap(ht, rows, mask, None, *planes, **kw), cc.restate_cap(rows, mask, None, *planes, **kw), base)


def test_a_array_form_of_the_restatement_equals_the_loop():
    for L, seed in ((1, 1), (7, 2), (65, 3), (200, 4)):
        rows, mask, seg = mc.random_rows(12, L, seed)
        for long_units in (False, True):
            S, E = mc.word_planes(12, L, seed, long_units)
            for planes in ((None, None), (S, E)):
                h, sel, w3 = cc.selection(rows, mask, seg, *planes, special_ids=[mc.CLS], probs=(0.4, 0.8, 0.1), seed=seed)
                for P in (0, 1, 2, 5, L // 4 + 1, L):
                    assert np.array_equal(cc.kept_loop(h, sel, w3, P), cc.kept_array(h, sel, w3, P)), (L, P)
                    if P:
                        kw = dict(special_ids=[mc.CLS], probs=(0.4, 0.8, 0.1), seed=seed, max_pred=P)
                        same(cc.restate_cap(rows, mask, seg, *planes, heads_fn=mc.heads_array, kept_fn=cc.kept_array, **kw), cc.restate_cap(rows, mask, seg, *planes, **kw), (L, P))
    # equal W3, different heads: the array form breaks the tie by the head too
    h = np.array([[0, 1, 2, 3]]); sel = np.ones((1, 4), dtype=bool); w3 = np.array([[7, 7, 7, 7]], dtype=np.uint64)
    for P in (1, 2, 3, 4):
        assert cc.kept_loop(h, sel, w3, P)[0].tolist() == cc.kept_array(h, sel, w3, P)[0].tolist() == [j < P for j in range(4)]


# ---- (b) the search alone, keys by hand
@pytest.mark.parametrize("G", GROUPS)
def test_b_the_search_on_hand_made_keys(ht, G):
    assert ht.bft_mlmcap_key(0xFFFFFFFF, 4095) == key(0xFFFFFFFF, 4095) and ht.bft_mlmcap_key(1, 0) == 1 << 32
    # equal W[3], different heads: the tie falls to the smaller head
    w = [key(9, 0), key(9, 1), key(9, 2), key(9, 3)]
    assert search(ht, w, 2, G) == [True, True, False, False] and search(ht, w[::-1], 1, G) == [False, False, False, True]
    # units 0-1 (W3 5), 2 (5), 3-5 (1), 7 (9); cell 6 unselected.  In key order 3-5, 0-1, 2, 7: prefix sums 3, 5, 6, 7
    w = [key(5, 0), key(5, 0), key(5, 2), key(1, 3), key(1, 3), key(1, 3), NONE, key(9, 7)]
    k = lambda *cells: [j in cells for j in range(8)]
    assert search(ht, w, 3, G) == k(3, 4, 5)                                       # P exactly a prefix sum
    assert search(ht, w, 2, G) == k()                                              # one less: the first unit does not fit, nothing is kept
    assert search(ht, w, 5, G) == k(0, 1, 3, 4, 5) and search(ht, w, 4, G) == k(3, 4, 5)          # the cut: cell 2 would fit at P = 4 and is not taken
    assert search(ht, w, 6, G) == k(0, 1, 2, 3, 4, 5) and search(ht, w, 7, G) == search(ht, w, 50, G) == k(0, 1, 2, 3, 4, 5, 7)
    # a unit larger than P with the smallest key: nothing is kept; with the largest key: everything in front of it
    big_first = [key(0, 0)] * 5 + [key(3, 5), key(4, 6)]
    assert search(ht, big_first, 4, G) == [False] * 7 and search(ht, big_first, 5, G) == [True] * 5 + [False] * 2
    big_last = [key(0xFFFFFFFF, 0)] * 5 + [key(3, 5), key(4, 6)]
    assert search(ht, big_last, 4, G) == [False] * 5 + [True] * 2 and search(ht, big_last, 6, G) == [False] * 5 + [True] * 2
    # all selected (one key per cell, keys falling along the row; 130 cells: three chunks at G = 64), none selected
    L = 130
    w = [key(1000 - j, j) for j in range(L)]
    for P in (1, 63, 64, 65, 129):
        assert search(ht, w, P, G) == [j >= L - P for j in range(L)], P
    assert search(ht, w, L, G) == [True] * L and search(ht, [NONE] * L, 1, G) == [False] * L
    # keys that differ in the lowest head bit alone, and in the highest bit of W[3] alone
    assert search(ht, [key(5, 1), key(5, 0)], 1, G) == [False, True]
    assert search(ht, [key(0x80000000, 0), key(0x7FFFFFFF, 1), key(0, 2)], 2, G) == [False, True, True]


# ---- (c) the inputs prove something; the rule itself
TABLE_BIG = [L for L in mc.TABLE_L if L >= 31]


@pytest.mark.parametrize("L", TABLE_BIG)
def test_c_the_table_inputs_take_both_branches(L):
    """257 rows, probabilities (0.3, 0.8, 0.1), seed 7, P = max(1, L // 8): the cap drops a unit in 0.34 .. 0.55 of the rows and leaves 0.31 .. 0.51 of
    them untouched with something selected (token and whole-word form, every L >= 31 of the table); at least a quarter each way is asserted"""
    rows, mask, seg, S, E = cc.table_inputs(L)
    for planes in ((None, None), (S, E)):
        binds, free, _ = cc.shares(rows, mask, seg, *planes, max(1, L // 8), special_ids=cc.TABLE_SPECIALS, probs=cc.PROBS, seed=7)
        print("L %d %s: binds %.3f free %.3f" % (L, "whole words" if planes[0] is not None else "tokens", binds, free))
        assert binds >= 0.25 and free >= 0.25, (L, binds, free)


@pytest.mark.parametrize("L", TABLE_BIG)
def test_c_a_first_unit_too_large_blocks_the_row(L):
    rows, mask, seg, S, E = cc.table_inputs(L)
    for P in (1, 2):
        _, _, blocked = cc.shares(rows, mask, seg, S, E, P, special_ids=cc.TABLE_SPECIALS, probs=cc.PROBS, seed=7)
        print("L %d P %d: blocked %.3f" % (L, P, blocked))
        assert blocked >= 0.04, (L, P, blocked)


@pytest.mark.parametrize("L", [33, 130])
def test_c_units_stay_whole(ht, L):
    rows, mask, seg, S, E = cc.table_inputs(L, 64)
    runs = mc.unit_runs(mc.heads(mc.eligible(rows, mask, seg, cc.TABLE_SPECIALS), S, E))
    assert sum(len(x) for x in runs) > 100
    for P in cc.table_P(L):
        kw = dict(special_ids=cc.TABLE_SPECIALS, probs=cc.PROBS, seed=7, max_pred=P)
        want = cc.restate_cap(rows, mask, seg, S, E, **kw)
        same(host_cap(ht, rows, mask, seg, S, E, **kw), want, (L, P))
        lab = want[1] != -100
        assert all(lab[r, a:z + 1].all() or not lab[r, a:z + 1].any() for r, rr in enumerate(runs) for a, z in rr)


@pytest.mark.parametrize("seed", [1, 12345, 0])
def test_c_no_position_is_preferred(seed):
    """4096 rows of 64 eligible cells, selection 0.5, P = 8: every row keeps exactly 8 cells, and each quarter of the row holds its share of
    them, 0.125 of its cells (0.1215 .. 0.1269 over these seeds); asserted within 0.01"""
    rows = np.full((4096, 64), 7, dtype=np.int32)
    h, sel, w3 = cc.selection(rows, probs=(0.5, 0.8, 0.1), seed=seed)
    kept = cc.kept_array(h, sel, w3, 8)
    assert (kept.sum(axis=1) == 8).all()
    share = [kept[:, q * 16:(q + 1) * 16].mean() for q in range(4)]
    print("seed %d: %s" % (seed, " ".join("%.4f" % x for x in share)))
    assert all(abs(x - 0.125) <= 0.01 for x in share)


# ---- (d) the base call
@pytest.mark.parametrize("L", [4, 33, 65, 130])
def test_d_no_cap_and_a_cap_nothing_reaches_are_the_base_call(ht, L):
    rows, mask, seg, S, E = cc.table_inputs(L, 40)
    for planes in ((None, None), (S, E)):
        kw = dict(special_ids=cc.TABLE_SPECIALS, probs=cc.PROBS, seed=3, epoch=1)
        base = mc.restate_mlm(rows, mask, seg, *planes, **kw)
        most = int((base[1] != -100).sum(axis=1).max())
        zero = cc.restate_cap(rows, mask, seg, *planes, max_pred=0, **kw)
        assert np.array_equal(zero[0], base[0]) and np.array_equal(zero[1], base[1]) and np.array_equal(zero[4], (base[1] != -100).sum(axis=1))
        for P in (most, most + 1, L + 5):
            for out in (cc.restate_cap(rows, mask, seg, *planes, max_pred=P, **kw), host_cap(ht, rows, mask, seg, *planes, max_pred=P, **kw)):
                assert np.array_equal(out[0], base[0]) and np.array_equal(out[1], base[1]), (L, P)
        if most > 1:
            out = host_cap(ht, rows, mask, seg, *planes, max_pred=most - 1, **kw)
            assert not np.array_equal(out[1], base[1])


@pytest.mark.parametrize("L", [31, 65, 200])
def test_d_labels_and_gathered_outputs_agree(ht, L):
    rows, mask, seg, S, E = cc.table_inputs(L, 50)
    for planes in ((None, None), (S, E)):
        for P in cc.table_P(L):
            ids, labels, cells, plabels, count = host_cap(ht, rows, mask, seg, *planes, special_ids=cc.TABLE_SPECIALS, probs=cc.PROBS, seed=5, max_pred=P)
            assert np.array_equal(count, (labels != -100).sum(axis=1)) and (count <= P).all()
            for r in range(len(rows)):
                k = int(count[r])
                assert np.array_equal(labels[r, cells[r, :k]], plabels[r, :k]) and np.array_equal(rows[r, cells[r, :k]], plabels[r, :k])
                assert (np.diff(cells[r, :k]) > 0).all() and (cells[r, k:] == 0).all() and (plabels[r, k:] == -100).all()


# ---- (e) declared and exported; the stand-alone program
def test_e_new_symbol_is_declared_and_exported():
    import blingfire_amd as bf
    hdr = open(os.path.join(bfutil.ROOT, "include", "blingfiretokdll_amd.h")).read()
    exports = open(os.path.join(bfutil.ROOT, "blingfire_amd", "csrc", "exports.map")).read()
    lib = ctypes.CDLL(bf.LIB_PATH)
    name = "RowsMlmPredictionsBatchDevice"
    assert re.search(r"BF_API\s+\w+\s+%s\(" % name, hdr)
    assert re.search(r"^\s*%s;" % name, exports, flags=re.M)
    assert hasattr(lib, name)
    assert re.search(r"#define\s+BF_MLM_CAP_MAX_LEN\s+4096\b", hdr)
    assert "max_predictions" in inspect.signature(bf.rows_mlm_mask_device).parameters
    assert "max_predictions" in inspect.signature(bf.encode_mlm_batch_device).parameters


def test_stand_alone_program_under_sanitizers(tmp_path):
    """the lane-code driver with its own main, built with -fsanitize=address,undefined and run as a program (never loaded into python)"""
    exe = str(tmp_path / "bf_mlmcaptest")
    src = os.path.join(bfutil.ROOT, "tests", "hosttest", "bf_mlmcaptest.cpp")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-DBF_MLMCAPTEST_MAIN", src, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("mlmcap ok:"), r.stdout + r.stderr
