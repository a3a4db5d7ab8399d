"""CPU tier of IdsToPairRowsBatch: the pair-row logic of blingfire_amd/csrc/bf_pairs.h -- the code the kernels run per lane -- compiled for the
host (tests/hosttest/bf_pairstest.cpp) against the numpy restatement of the specification (pair_cases.restate), and the same file as a
program of its own under the address and undefined-behaviour sanitizers."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import bfutil
import pair_cases as pc

c_i64, c_int, c_vp = ctypes.c_int64, ctypes.c_int, ctypes.c_void_p


@pytest.fixture(scope="module")
def ht():
    L = ctypes.CDLL(bfutil.HOSTTEST_LIB)
    L.bft_pair_rows_batch.restype = c_i64
    L.bft_pair_rows_batch.argtypes = [c_vp, c_i64, c_vp, c_vp, c_i64, c_vp, c_i64] + [c_int] * 9 + [c_vp] * 5 + [c_i64, c_vp, ctypes.POINTER(c_int)]
    return L


CANARY32, CANARY8 = -0x35014542, 0xA5
CANARIES = (CANARY32, CANARY8, CANARY8, CANARY32, CANARY32)


def host_pairs(ht, src, par, rows_cap, pad_id=pc.PAD, len_a=None, len_b=None, want=(True,) * 5):
    """bft_pair_rows_batch over canary-filled arrays of rows_cap rows -> (total, [rows, mask, type, seq, first], offsets, status)"""
    L, cls_id, sep_id, double_sep, mode, max_a, stride, max_rows, pad_left = par
    ids_a, off_a, ids_b, off_b = (np.ascontiguousarray(x, dtype=t) for x, t in zip(src, (np.int32, np.int64, np.int32, np.int64)))
    W = max(L, 0)
    outs = [np.full((rows_cap, W), CANARY32, dtype=np.int32), np.full((rows_cap, W), CANARY8, dtype=np.uint8), np.full((rows_cap, W), CANARY8, dtype=np.uint8),
            np.full(rows_cap, CANARY32, dtype=np.int32), np.full(rows_cap, CANARY32, dtype=np.int32)]
    r_off = np.full(len(off_a), -1, dtype=np.int64)
    status = c_int(-1)
    ptr = [a.ctypes.data if w else None for a, w in zip(outs, want)]
    total = ht.bft_pair_rows_batch(ids_a.ctypes.data, len(ids_a) if len_a is None else len_a, off_a.ctypes.data, ids_b.ctypes.data, len(ids_b) if len_b is None else len_b,
                                   off_b.ctypes.data, len(off_a) - 1, L, cls_id, sep_id, pad_id, mode, max_a, stride, max_rows, pc.flags(pad_left, double_sep), *ptr,
                                   rows_cap, r_off.ctypes.data, ctypes.byref(status))
    return total, outs, r_off, status.value


def restate(src, par, **kw):
    L, cls_id, sep_id, double_sep, mode, max_a, stride, max_rows, pad_left = par
    return pc.restate(*src, L, cls_id, sep_id, pc.PAD, mode, max_a, stride, max_rows, pad_left, double_sep, **kw)


def test_the_table_has_every_combination():
    t = pc.table()
    assert {p[0] for p in t} == set(pc.TABLE_L) and {p[4] for p in t} == {0, 1} and {p[8] for p in t} == {False, True}
    assert {p[7] for p in t if p[4] == 0} == {0, 1, 2, 3}
    for L in pc.TABLE_L:
        kinds = {(c >= 0, s >= 0, d) for l, c, s, d, *_ in t if l == L}
        full = {(c, s, d) for c in (True, False) for s, d in ((False, False), (True, False), (True, True))}
        assert kinds == (full if L > 4 else full - {(True, True, True)}), L      # L = 4 has no room behind four specials
        for c, s, d in kinds:
            T = L - c - (s + d + 1 if s else 0)
            mine = [p for p in t if p[0] == L and (p[1] >= 0, p[2] >= 0, p[3]) == (c, s, d)]
            assert {p[5] for p in mine if p[4] == 0} == {0, 1, T - 1} & set(range(T))
            for max_a in {p[5] for p in mine if p[4] == 0}:
                assert {p[6] for p in mine if p[4] == 0 and p[5] == max_a} == {0, 1, T - max_a - 1} & set(range(T - max_a))
    assert any(p[4] == 1 and pc.room(*p[:4]) % 2 == 1 for p in t)            # mode 1 at an odd T
    for p in t[::17]:                                                        # the pair lengths are the ones the table names
        lens = pc.pair_lengths(p)
        if p[4] == 1:
            T = pc.room(*p[:4])
            ns = {0, 1, T // 2, (T + 1) // 2, (T + 1) // 2 + 1, T, T + 1, 3 * T}
            assert set(lens) == {(a, b) for a in ns for b in ns}
        else:
            assert {na for na, _ in lens} == {na for na in (0, 1, p[5] - 1, p[5], p[5] + 1) if na >= 0}
            assert all(sum(1 for a, _ in lens if a == na) % 8 == 0 for na in {na for na, _ in lens})


@pytest.mark.parametrize("L", pc.TABLE_L)
def test_lane_code_equals_the_restatement(ht, L):
    n = 0
    for par in pc.table():
        if par[0] != L:
            continue
        src = pc.synthetic(par, seed=n)
        want = restate(src, par)
        total = len(want[3])
        for cap in sorted({0, max(total - 1, 0), total, total + 1}):
            got = host_pairs(ht, src, par, cap)
            assert got[0] == total and np.array_equal(got[2], want[5]), (par, cap)
            k = min(cap, total)
            for g, w, can in zip(got[1], want[:5], CANARIES):
                assert g.dtype == w.dtype and np.array_equal(g[:k], w[:k]) and (g[k:] == can).all(), (par, cap)
            assert got[3] == (1 if total > cap else 0), (par, cap)
        n += 1
    assert n > 0


def test_closed_form_of_longest_first_equals_the_loop(ht):
    """every T < 20 with na, nb < 45: the lane code (closed form) against the drop-one-id loop of the restatement; and both inputs cut to T
    ids first give the same rows"""
    ns = [(a, b) for a in range(45) for b in range(45)]
    ids_a, off_a = pc.ragged([a for a, _ in ns], pc.A0)
    ids_b, off_b = pc.ragged([b for _, b in ns], pc.B0)
    for T in range(1, 20):
        for par in ((T, -1, -1, False, 1, 0, 0, 1, False), (T + 3, pc.CLS, pc.SEP, False, 1, 0, 0, 1, True)):
            want = restate((ids_a, off_a, ids_b, off_b), par)
            got = host_pairs(ht, (ids_a, off_a, ids_b, off_b), par, len(ns))
            assert got[0] == len(ns) and got[3] == 0
            for g, w in zip(got[1], want[:5]):
                assert np.array_equal(g, w), T
            cut_a = [ids_a[off_a[q]:off_a[q + 1]][:T] for q in range(len(ns))]
            cut_b = [ids_b[off_b[q]:off_b[q + 1]][:T] for q in range(len(ns))]
            src = (np.concatenate(cut_a), np.cumsum([0] + [len(x) for x in cut_a]), np.concatenate(cut_b), np.cumsum([0] + [len(x) for x in cut_b]))
            cut = host_pairs(ht, src, par, len(ns))
            assert np.array_equal(cut[1][0], want[0]) and np.array_equal(cut[1][2], want[2])


BAD = [([0, 5, 3, 12, 20], 40), ([0, 10, 50, 50, 60], 40), ([0, 10, 20, 30, 40], 25), ([-1, 4, 9, 12, 13], 40)]
GOOD = ([0, 3, 9, 9, 30], 40)


@pytest.mark.parametrize("par", [(8, pc.CLS, pc.SEP, False, 0, 2, 1, 0, False), (9, pc.CLS, pc.SEP, True, 1, 0, 0, 1, True)])
def test_bad_ranges_make_that_side_empty(ht, par):
    ids_a = np.arange(pc.A0, pc.A0 + 40, dtype=np.int32); ids_b = np.arange(pc.B0, pc.B0 + 40, dtype=np.int32)
    for (oa, la), (ob, lb) in [(b, GOOD) for b in BAD] + [(GOOD, b) for b in BAD] + [(BAD[0], BAD[1]), (BAD[2], BAD[3])]:
        src = (ids_a, oa, ids_b, ob)
        want = restate(src, par, len_a=la, len_b=lb)
        assert want[6] == 8
        got = host_pairs(ht, src, par, len(want[3]), len_a=la, len_b=lb)
        assert got[0] == len(want[3]) and got[3] == 8 and np.array_equal(got[2], want[5])
        for g, w in zip(got[1], want[:5]):
            assert np.array_equal(g, w), (oa, ob)
    # the same array on both sides
    src = (ids_a, GOOD[0], ids_a, [0, 10, 20, 30, 40])
    want = restate(src, par)
    got = host_pairs(ht, src, par, len(want[3]))
    assert got[3] == 0 and all(np.array_equal(g, w) for g, w in zip(got[1], want[:5]))


def test_refused_parameters(ht):
    src = (np.arange(4, dtype=np.int32), [0, 4], np.arange(4, dtype=np.int32), [0, 4])

    def total(L=8, cls_id=1, sep_id=2, double_sep=False, mode=0, max_a=2, stride=1, max_rows=0, pad_left=False, cap=0):
        return host_pairs(ht, src, (L, cls_id, sep_id, double_sep, mode, max_a, stride, max_rows, pad_left), cap, want=(False,) * 5)[0]
    assert total() == 2 and total(mode=1, max_a=0, stride=0, max_rows=1) == 1
    for bad in (dict(L=0), dict(L=-1), dict(L=(1 << 20) + 1), dict(L=3), dict(L=4, double_sep=True), dict(L=1, sep_id=-1), dict(mode=2), dict(mode=-1),
                dict(max_a=-1), dict(max_a=5), dict(stride=-1), dict(stride=3), dict(max_a=4, stride=1), dict(max_rows=-1), dict(sep_id=-1, double_sep=True),
                dict(mode=1), dict(mode=1, max_a=1, stride=0, max_rows=1), dict(mode=1, max_a=0, stride=1, max_rows=1), dict(mode=1, max_a=0, stride=0, max_rows=0),
                dict(mode=1, max_a=0, stride=0, max_rows=2)):
        assert total(**bad) == -1, bad
    assert total(max_a=4, stride=0) == 4 and total(max_a=0, stride=4) == 1 and total(L=4, max_a=0, stride=0) == 4 and total(L=1 << 20) == 1
    assert total(L=1, cls_id=-1, sep_id=-1, max_a=0, stride=0) == 4
    for flags in (4, 5, 8, 1 << 30, -1):
        st = c_int(0); r_off = np.zeros(2, dtype=np.int64); o = np.array([0, 4], dtype=np.int64)
        assert ht.bft_pair_rows_batch(src[0].ctypes.data, 4, o.ctypes.data, src[0].ctypes.data, 4, o.ctypes.data, 1, 8, 1, 2, 0, 0, 2, 1, 0, flags,
                                      None, None, None, None, None, 0, r_off.ctypes.data, ctypes.byref(st)) == -1, flags


def test_optional_outputs_and_size_query(ht):
    par = (8, pc.CLS, pc.SEP, False, 0, 2, 1, 0, False)
    src = pc.synthetic(par)
    want = restate(src, par)
    total = len(want[3])
    q = host_pairs(ht, src, par, 0, want=(False,) * 5)
    assert q[0] == total and q[3] == 0 and np.array_equal(q[2], want[5])
    for drop in range(5):
        w = tuple(i != drop for i in range(5))
        got = host_pairs(ht, src, par, total, want=w)
        for i in range(5):
            assert np.array_equal(got[1][i], want[i]) if w[i] else (got[1][i] == CANARIES[i]).all()


def test_count_saturates_at_int32_max(ht):
    """one B of 2^31 + 10 ids at T = 1 (no id is read by a size query): INT32_MAX rows and status bit 0"""
    off_a = np.zeros(3, dtype=np.int64)
    off_b = np.array([0, (1 << 31) + 10, (1 << 31) + 11], dtype=np.int64)
    r_off = np.zeros(3, dtype=np.int64); st = c_int(0)
    total = ht.bft_pair_rows_batch(None, 0, off_a.ctypes.data, None, (1 << 31) + 11, off_b.ctypes.data, 2, 1, -1, -1, 0, 0, 0, 0, 0, 0,
                                   None, None, None, None, None, 0, r_off.ctypes.data, ctypes.byref(st))
    assert total == pc.INT32_MAX + 1 and list(r_off) == [0, pc.INT32_MAX, pc.INT32_MAX + 1] and st.value == 1


def test_array_form_of_the_restatement_equals_the_row_form():
    rnd = np.random.RandomState(5)
    for L in (4, 9, 64):
        T = L - 3
        la = np.concatenate([[0, 1, T, T + 1, 3 * L, 0], rnd.randint(0, 2 * L, size=300)])
        lb = np.concatenate([[0, T, 1, T + 1, 3 * L, 3 * L], rnd.randint(0, 2 * L, size=300)])
        ids_a, off_a = pc.ragged(la, pc.A0)
        ids_b, off_b = pc.ragged(lb, pc.B0)
        for mode, max_a in ((1, 0), (0, 0), (0, T // 2), (0, T - 1)):
            want = pc.restate(ids_a, off_a, ids_b, off_b, L, pc.CLS, pc.SEP, pc.PAD, mode, max_a, 0, 1)
            for a, b in zip(pc.restate_one_row(ids_a, off_a, ids_b, off_b, L, pc.CLS, pc.SEP, pc.PAD, mode, max_a, chunk=100), want[:6]):
                assert a.dtype == b.dtype and np.array_equal(a, b), (L, mode, max_a)


def test_stand_alone_program_under_sanitizers(tmp_path):
    """the same file with its own main, built with -fsanitize=address,undefined and run as a program (never loaded into python)"""
    exe = str(tmp_path / "bf_pairstest")
    src = os.path.join(bfutil.ROOT, "tests", "hosttest", "bf_pairstest.cpp")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-DBF_PAIRSTEST_MAIN", src, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("pairs ok:"), r.stdout + r.stderr
