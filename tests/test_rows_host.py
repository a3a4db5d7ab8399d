"""CPU tier of IdsToRowsBatch: the row logic of blingfire_amd/csrc/bf_rows.h -- the code the kernels run per lane -- compiled for the host
(tests/hosttest/bf_rowstest.cpp) against the numpy restatement of the specification (rows_cases.restate), the same file as a program of
its own under the address and undefined-behaviour sanitizers, and the stored reference ids of the end-to-end GPU cases against the
live reference where it is built."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import bfutil
import rows_cases as rc

c_i64, c_int, c_vp = ctypes.c_int64, ctypes.c_int, ctypes.c_void_p


@pytest.fixture(scope="module")
def ht():
    L = ctypes.CDLL(bfutil.HOSTTEST_LIB)
    L.bft_rows_batch.restype = c_i64
    L.bft_rows_batch.argtypes = [c_vp, c_i64, c_vp, c_i64, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_vp, c_vp, c_vp, c_vp, c_i64, c_vp, ctypes.POINTER(c_int)]
    return L


CANARY32, CANARY8 = -0x35014542, 0xA5


def host_rows(ht, ids, off, L, cls_id, sep_id, pad_id, stride, max_rows, pad_left, rows_cap, ids_len=None, want=(True, True, True, True)):
    """bft_rows_batch over canary-filled arrays of rows_cap rows -> (total, rows, mask, seq, first, offsets, status)"""
    ids = np.ascontiguousarray(ids, dtype=np.int32); off = np.ascontiguousarray(off, dtype=np.int64)
    rows = np.full((rows_cap, L), CANARY32, dtype=np.int32); mask = np.full((rows_cap, L), CANARY8, dtype=np.uint8)
    seq = np.full(rows_cap, CANARY32, dtype=np.int32); first = np.full(rows_cap, CANARY32, dtype=np.int32)
    r_off = np.full(len(off), -1, dtype=np.int64)
    status = c_int(-1)
    ptr = [a.ctypes.data if w else None for a, w in zip((rows, mask, seq, first), want)]
    total = ht.bft_rows_batch(ids.ctypes.data, len(ids) if ids_len is None else ids_len, off.ctypes.data, len(off) - 1, L, cls_id, sep_id, pad_id, stride,
                              max_rows, 1 if pad_left else 0, *ptr, rows_cap, r_off.ctypes.data, ctypes.byref(status))
    return total, rows, mask, seq, first, r_off, status.value


def test_the_table_has_every_combination():
    t = rc.table()
    assert {p[0] for p in t} == set(rc.TABLE_L) and {p[4] for p in t} == {0, 1, 2, 3} and {p[5] for p in t} == {False, True}
    assert all(c == -1 and s == -1 for L, c, s, *_ in t if L == 1)
    for L in rc.TABLE_L[3:]:
        assert {(c >= 0, s >= 0) for l, c, s, *_ in t if l == L} == {(True, True), (True, False), (False, True), (False, False)}
        body = L - 2
        assert {p[3] for p in t if p[0] == L and p[1] >= 0 and p[2] >= 0} == {0, 1, body - 1}


@pytest.mark.parametrize("L", rc.TABLE_L)
def test_lane_code_equals_the_restatement(ht, L):
    n = 0
    for (l, cls_id, sep_id, stride, max_rows, pad_left) in rc.table():
        if l != L:
            continue
        body, step = rc.geometry(L, cls_id, sep_id, stride)
        ids, off = rc.synthetic(body, step, seed=n)
        want = rc.restate(ids, off, L, cls_id, sep_id, rc.PAD, stride, max_rows, pad_left)
        total = len(want[2])
        for cap in sorted({0, max(total - 1, 0), total, total + 1}):
            got = host_rows(ht, ids, off, L, cls_id, sep_id, rc.PAD, stride, max_rows, pad_left, cap)
            key = (L, cls_id, sep_id, stride, max_rows, pad_left, cap)
            assert got[0] == total and np.array_equal(got[5], want[4]), key
            k = min(cap, total)
            for g, w in zip(got[1:5], want[:4]):
                assert np.array_equal(g[:k], w[:k]), key
            assert (got[1][k:] == CANARY32).all() and (got[2][k:] == CANARY8).all() and (got[3][k:] == CANARY32).all() and (got[4][k:] == CANARY32).all(), key
            assert got[6] == (1 if total > cap else 0), key
        n += 1
    assert n > 0


def test_bad_ranges_are_empty_sequences(ht):
    ids = np.arange(1000, 1040, dtype=np.int32)
    for off, ids_len in (([0, 5, 3, 12, 20], 40), ([0, 10, 50, 50, 60], 40), ([0, 10, 20, 30, 40], 25), ([-1, 4, 9], 40)):
        want = rc.restate(ids, off, 8, rc.CLS, rc.SEP, rc.PAD, 2, 0, False, ids_len=ids_len)
        assert want[5] == 8
        got = host_rows(ht, ids, off, 8, rc.CLS, rc.SEP, rc.PAD, 2, 0, False, len(want[2]), ids_len=ids_len)
        assert got[0] == len(want[2]) and got[6] == 8
        for g, w in zip(got[1:6], want[:5]):
            assert np.array_equal(g, w), (off, ids_len)


def test_refused_parameters(ht):
    ids, off = np.arange(4, dtype=np.int32), [0, 4]
    ok = dict(L=8, cls_id=1, sep_id=2, pad_id=0, stride=0, max_rows=1, pad_left=False, rows_cap=1)
    assert host_rows(ht, ids, off, **ok)[0] == 1
    for bad in (dict(L=0), dict(L=(1 << 20) + 1), dict(L=2), dict(L=1, sep_id=-1), dict(stride=-1), dict(stride=6), dict(max_rows=-1)):
        assert host_rows(ht, ids, off, **dict(ok, **bad, rows_cap=0))[0] == -1, bad
    assert host_rows(ht, ids, off, **dict(ok, L=1, cls_id=-1, sep_id=-1, rows_cap=1))[0] == 1
    r_off = np.zeros(2, dtype=np.int64); st = c_int(0)
    for flags in (2, 3, 4, 1 << 30):
        assert ht.bft_rows_batch(ids.ctypes.data, 4, np.array(off, dtype=np.int64).ctypes.data, 1, 8, 1, 2, 0, 0, 1, flags, None, None, None, None, 0, r_off.ctypes.data, ctypes.byref(st)) == -1


def test_optional_outputs_and_size_query(ht):
    ids, off = rc.synthetic(6, 4)
    want = rc.restate(ids, off, 8, rc.CLS, rc.SEP, rc.PAD, 2, 0, False)
    total = len(want[2])
    q = host_rows(ht, ids, off, 8, rc.CLS, rc.SEP, rc.PAD, 2, 0, False, 0, want=(False,) * 4)
    assert q[0] == total and q[6] == 0 and np.array_equal(q[5], want[4])
    for drop in range(4):
        w = tuple(i != drop for i in range(4))
        got = host_rows(ht, ids, off, 8, rc.CLS, rc.SEP, rc.PAD, 2, 0, False, total, want=w)
        for i in range(4):
            assert np.array_equal(got[1 + i], want[i]) if w[i] else (got[1 + i] == (CANARY8 if i == 1 else CANARY32)).all()


def test_count_saturates_at_int32_max(ht):
    """one sequence of 2^31 + 10 ids at body 1, step 1 (no id is read by a size query): INT32_MAX rows and status bit 0"""
    off = np.array([0, (1 << 31) + 10, (1 << 31) + 11], dtype=np.int64)
    r_off = np.zeros(3, dtype=np.int64); st = c_int(0)
    total = ht.bft_rows_batch(None, (1 << 31) + 11, off.ctypes.data, 2, 1, -1, -1, 0, 0, 0, 0, None, None, None, None, 0, r_off.ctypes.data, ctypes.byref(st))
    assert total == rc.INT32_MAX + 1 and list(r_off) == [0, rc.INT32_MAX, rc.INT32_MAX + 1] and st.value == 1


def test_array_form_of_the_restatement_equals_the_row_form():
    rnd = np.random.RandomState(3)
    for L in (3, 8, 64):
        lens = np.concatenate([[0, 1, L - 3, L - 2, L - 1, 3 * L], rnd.randint(0, 2 * L, size=200)])
        off = np.zeros(len(lens) + 1, dtype=np.int64); np.cumsum(lens, out=off[1:])
        ids = rnd.randint(1000, 30000, size=int(off[-1])).astype(np.int32)
        for a, b in zip(rc.restate_truncated(ids, off, L, rc.CLS, rc.SEP, rc.PAD), rc.restate(ids, off, L, rc.CLS, rc.SEP, rc.PAD)[:5]):
            assert a.dtype == b.dtype and np.array_equal(a, b)


def test_stand_alone_program_under_sanitizers(tmp_path):
    """the same file with its own main, built with -fsanitize=address,undefined and run as a program (never loaded into python)"""
    exe = str(tmp_path / "bf_rowstest")
    src = os.path.join(bfutil.ROOT, "tests", "hosttest", "bf_rowstest.cpp")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-DBF_ROWSTEST_MAIN", src, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("rows ok:"), r.stdout + r.stderr


def test_fixture_shape_and_live_reference():
    fx = rc.load_fixture()
    docs = rc.encode_docs()
    assert fx["docs"] == len(docs) == len(bfutil.ADVERSARIAL) + 48
    lens = sorted({rc.encode_max_len(L, s, r) for L, s, r, _ in rc.ENCODE_CASES})
    assert lens == [6, 14, rc.INT32_MAX]
    for model in rc.ENCODE_MODELS:
        assert sorted(int(k) for k in fx["models"][model]) == lens
        for m in lens:
            per_doc = fx["models"][model][str(m)]
            assert len(per_doc) == len(docs) and all(len(d) <= m for d in per_doc)
    if bfutil.have_ref():
        import importlib.util
        spec = importlib.util.spec_from_file_location("make_rows_fixture", os.path.join(bfutil.ROOT, "tests", "golden", "make_rows_fixture.py"))
        mod = importlib.util.module_from_spec(spec); spec.loader.exec_module(mod)
        assert mod.compute() == fx, "tests/golden/rows/encode_ids.json differs from the live reference"
