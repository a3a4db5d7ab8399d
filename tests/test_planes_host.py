"""CPU tier of the companion planes and the span cells (IdsToRowsPlanesBatch, IdsToPairRowsPlanesBatch, RowsSpanCellsBatchDevice): rows written out by
hand from the specification pin the restatements of plane_cases; the lane code of blingfire_amd/csrc/bf_rows.h / bf_pairs.h -- the "where" calls
and the span predicate and combine, compiled for the host (tests/hosttest/bf_planestest.cpp) -- is held to those restatements over both
parameter tables; and the new symbols are declared and exported."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import bfutil
import pair_cases as pc
import plane_cases as pl
import rows_cases as rc

c_i64, c_int, c_vp = ctypes.c_int64, ctypes.c_int, ctypes.c_void_p
CANARY32 = pl.CANARY32
NEW_SYMBOLS = ["IdsToRowsPlanesBatchDevice", "IdsToRowsPlanesBatch", "IdsToPairRowsPlanesBatchDevice", "IdsToPairRowsPlanesBatch", "RowsSpanCellsBatchDevice"]


@pytest.fixture(scope="module")
def ht():
    L = ctypes.CDLL(bfutil.HOSTTEST_LIB)
    L.bft_rows_planes.restype = c_i64
    L.bft_rows_planes.argtypes = [c_vp, c_i64, c_vp, c_i64] + [c_int] * 7 + [c_vp] * 3 + [c_i64, c_vp, ctypes.POINTER(c_int)]
    L.bft_pair_rows_planes.restype = c_i64
    L.bft_pair_rows_planes.argtypes = [c_vp, c_i64, c_vp, c_vp, c_i64, c_vp, c_i64] + [c_int] * 9 + [c_vp] * 4 + [c_i64, c_vp, ctypes.POINTER(c_int)]
    L.bft_span_group.restype = c_int
    L.bft_span_group.argtypes = [c_int]
    L.bft_span_rows.restype = c_int
    L.bft_span_rows.argtypes = [c_vp, c_vp, c_int, c_i64, c_vp, c_i64, c_vp, c_vp, c_int, c_vp, c_vp, c_int]
    return L


def ptr_array(arrays, n):
    return (c_vp * max(n, 1))(*[None if a is None else a.ctypes.data for a in arrays])


# ---- (a) literal examples: the restatements against rows written out by hand from the header text
X = -1          # the fill of the examples below


def test_a_rows_left_padded_windows_by_hand():
    """L = 6 with both specials: body 4; stride 1: step 3; every window; the padding first.  Sequence 0 has 2 ids, sequence 1 has 6 (two windows:
    ids 0 .. 3, then ids 3 .. 5)."""
    off = [0, 2, 8]
    starts = [0, 4, 0, 2, 5, 9, 12, 15]
    ends = [2, 8, 1, 3, 7, 10, 13, 18]
    planes, seq, first, r_off, st = pl.restate_planes(off, 6, rc.CLS, rc.SEP, 1, 0, True, [starts, ends], [X, X])
    assert st == 0 and seq.tolist() == [0, 1, 1] and first.tolist() == [0, 0, 3] and r_off.tolist() == [0, 1, 3]
    assert planes[0].tolist() == [[X, X, X, 0, 4, X],        # pad pad cls id0 id1 sep
                                  [X, 0, 2, 5, 9, X],        # cls id0 .. id3 sep
                                  [X, X, 9, 12, 15, X]]      # pad cls id3 id4 id5 sep
    assert planes[1].tolist() == [[X, X, X, 2, 8, X], [X, 1, 3, 7, 10, X], [X, X, 10, 13, 18, X]]
    S, E = planes

    def cells(a0, z0, a1, z1, none=0):
        s, e, status = pl.restate_span(S, E, seq, 2, [a0, a1], [z0, z1], none)
        assert status == 0
        return list(zip(s.tolist(), e.tolist()))
    # the answer of sequence 1 is its ids 3 and 4 (bytes 9 .. 13): it straddles the edge of window 0 (id 4 is not there), window 1 holds it
    assert cells(4, 8, 9, 13) == [(4, 4), (0, 0), (2, 3)]
    # an answer inside the gaps between tokens (bytes 4 .. 8 of sequence 1: behind id 1, in front of id 3) takes the tokens around it
    assert cells(0, 1, 4, 8) == [(3, 3), (2, 4), (0, 0)]
    # no span (a < 0), an inverted one (z < a), and another none_cell
    assert cells(-1, 5, 9, 8, none=-100) == [(-100, -100)] * 3
    # before every token of a window / behind every token
    assert cells(0, 0, 0, 1) == [(3, 3), (1, 1), (0, 0)] and cells(9, 9, 19, 19) == [(0, 0)] * 3


def test_a_pair_rows_double_separator_by_hand():
    """L = 9: cls, two middle separators, a trailing one: T = 5; mode 0 with max_a 2 and stride 1; the pair has 3 ids in A (2 are kept) and 4 in B:
    body_b 3, step 2, two windows (B ids 0 .. 2, then 2 .. 3).  Plane 0: B's starts alone, fill -5; plane 1: labels of A alone (one of them
    equal to the fill); plane 2: B's ends."""
    off_a, off_b = [0, 3], [0, 4]
    b_starts, b_ends, a_labels = [0, 3, 6, 10], [1, 4, 8, 12], [7, -1, 9]
    planes, seq, first, r_off, st = pl.restate_pair_planes(off_a, off_b, 9, pc.CLS, pc.SEP, 0, 2, 1, 0, False, True, src_a=[None, a_labels, None],
                                                           src_b=[b_starts, None, b_ends], fill=[-5, -1, -1])
    assert st == 0 and seq.tolist() == [0, 0] and first.tolist() == [0, 2] and r_off.tolist() == [0, 2]
    F = -5
    assert planes[0].tolist() == [[F, F, F, F, F, 0, 3, 6, F],       # cls a0 a1 sep sep b0 b1 b2 sep
                                  [F, F, F, F, F, 6, 10, F, F]]      # cls a0 a1 sep sep b2 b3 sep pad
    assert planes[1].tolist() == [[X, 7, -1, X, X, X, X, X, X]] * 2
    assert planes[2].tolist() == [[X] * 5 + [1, 4, 8, X], [X] * 5 + [8, 12, X, X]]
    # the answer is B's ids 2 and 3 (bytes 6 .. 12): window 0 ends inside it, window 1 holds it; the question's cells (fill) are never answer cells
    s, e, status = pl.restate_span(planes[0], planes[2], seq, 1, [6], [12], 0)
    assert status == 0 and list(zip(s.tolist(), e.tolist())) == [(0, 0), (5, 6)]
    # a row whose item is out of range: none_cell and bit 3; rows past the row count keep what they held
    s, e, status = pl.restate_span(planes[0], planes[2], [0, 1], 1, [6], [12], -100)
    assert status == 8 and s.tolist() == [-100, -100]
    s, e, status = pl.restate_span(planes[0], planes[2], None, 2, [6, 6], [12, 12], 0, nrows=1)
    assert s.tolist() == [0, CANARY32] and e.tolist() == [0, CANARY32]


def test_a_span_does_not_assume_an_order():
    S = np.array([[9, -1, 3, 7, 3, 0]], dtype=np.int32)
    E = np.array([[9, 50, 5, 8, 4, 2]], dtype=np.int32)
    # S <= 3 at cells 2, 4, 5: the last is 5; E >= 5 at cells 0, 2, 3 (cell 1 has no token): the first is 0
    s, e, _ = pl.restate_span(S, E, None, 1, [3], [5], 0)
    assert (s.tolist(), e.tolist()) == ([5], [0])


def test_a_array_form_of_the_restatement_equals_the_row_form():
    rnd = np.random.RandomState(3)
    lens = np.concatenate([[0, 1, 7, 8, 30, 0], rnd.randint(0, 14, size=200)])
    ids, off = pc.ragged(lens, 1000)
    src = pl.sources(len(ids), 2, 0, pl.FILLS)
    a = pl.restate_planes_truncated(off, 9, src, pl.FILLS[:2])
    b = pl.restate_planes(off, 9, rc.CLS, rc.SEP, 0, 1, False, src, pl.FILLS[:2])
    assert all(np.array_equal(x, y) for x, y in zip(a[0], b[0])) and all(np.array_equal(x, y) for x, y in zip(a[1:4], b[1:4]))


# ---- (b) the lane code against the restatements
def host_rows_planes(ht, ids, off, par, src, fill, cap, ids_len=None):
    L, cls_id, sep_id, stride, max_rows, pad_left = par
    off = np.ascontiguousarray(off, dtype=np.int64)
    n = len(fill)
    outs = [np.full((cap, L), CANARY32, dtype=np.int32) for _ in range(n)]
    r_off = np.full(len(off), -1, dtype=np.int64)
    status = c_int(-1)
    fills = (ctypes.c_int32 * max(n, 1))(*fill)
    total = ht.bft_rows_planes(ids.ctypes.data, len(ids) if ids_len is None else ids_len, off.ctypes.data, len(off) - 1, L, cls_id, sep_id, stride, max_rows,
                               1 if pad_left else 0, n, ptr_array(src, n), fills, ptr_array(outs, n), cap, r_off.ctypes.data, ctypes.byref(status))
    return total, outs, r_off, status.value


def host_pair_planes(ht, srcs, par, src_a, src_b, fill, cap):
    L, cls_id, sep_id, double_sep, mode, max_a, stride, max_rows, pad_left = par
    ids_a, off_a, ids_b, off_b = (np.ascontiguousarray(x, dtype=t) for x, t in zip(srcs, (np.int32, np.int64, np.int32, np.int64)))
    n = len(fill)
    outs = [np.full((cap, L), CANARY32, dtype=np.int32) for _ in range(n)]
    r_off = np.full(len(off_a), -1, dtype=np.int64)
    status = c_int(-1)
    fills = (ctypes.c_int32 * max(n, 1))(*fill)
    total = ht.bft_pair_rows_planes(ids_a.ctypes.data, len(ids_a), off_a.ctypes.data, ids_b.ctypes.data, len(ids_b), off_b.ctypes.data, len(off_a) - 1, L, cls_id, sep_id,
                                    mode, max_a, stride, max_rows, pc.flags(pad_left, double_sep), n, None if src_a is None else ptr_array(src_a, n),
                                    None if src_b is None else ptr_array(src_b, n), fills, ptr_array(outs, n), cap, r_off.ctypes.data, ctypes.byref(status))
    return total, outs, r_off, status.value


@pytest.mark.parametrize("L", rc.TABLE_L)
def test_b_rows_where_equals_the_restatement(ht, L):
    n = 0
    for par in rc.table():
        if par[0] != L:
            continue
        _, cls_id, sep_id, stride, max_rows, pad_left = par
        ids, off = rc.synthetic(*rc.geometry(L, cls_id, sep_id, stride), seed=n)
        nplanes = (1, 2, 4)[n % 3]
        fill = pl.FILLS[:nplanes]
        src = pl.sources(len(ids), nplanes, n, fill)
        want = pl.restate_planes(off, L, cls_id, sep_id, stride, max_rows, pad_left, src, fill)
        total = len(want[1])
        for cap in sorted({max(total - 1, 0), total}):
            got = host_rows_planes(ht, ids, off, par, src, fill, cap)
            assert got[0] == total and np.array_equal(got[2], want[3]) and got[3] == (1 if total > cap else 0), (par, cap)
            k = min(cap, total)
            for g, w in zip(got[1], want[0]):
                assert np.array_equal(g[:k], w[:k]) and (g[k:] == CANARY32).all(), (par, cap)
        n += 1
    assert n > 0


@pytest.mark.parametrize("L", pc.TABLE_L)
def test_b_pairs_where_equals_the_restatement(ht, L):
    n = 0
    for par in pc.table():
        if par[0] != L:
            continue
        _, cls_id, sep_id, double_sep, mode, max_a, stride, max_rows, pad_left = par
        srcs = pc.synthetic(par, seed=n)
        nplanes = (1, 2, 4)[n % 3]
        fill = pl.FILLS[:nplanes]
        src_a = pl.sources(len(srcs[0]), nplanes, n, fill)
        src_b = pl.sources(len(srcs[2]), nplanes, n + 1000, fill)
        sides = [(src_a, src_b), (src_a, None), (None, src_b), (None, None), ([None] + src_a[1:], src_b[:-1] + [None])][n % 5]
        want = pl.restate_pair_planes(srcs[1], srcs[3], L, cls_id, sep_id, mode, max_a, stride, max_rows, pad_left, double_sep, sides[0], sides[1], fill)
        total = len(want[1])
        got = host_pair_planes(ht, srcs, par, sides[0], sides[1], fill, total)
        assert got[0] == total and np.array_equal(got[2], want[3]) and got[3] == 0, par
        for g, w in zip(got[1], want[0]):
            assert np.array_equal(g, w), par
        n += 1
    assert n > 0


def test_b_bad_ranges_have_no_id_cells(ht):
    ids = (1000 + np.arange(40)).astype(np.int32)
    src = [np.arange(100, 140, dtype=np.int32)]
    for off, ids_len in (([0, 5, 3, 12, 20], 40), ([0, 10, 50, 50, 60], 40), ([0, 10, 20, 30, 40], 25), ([-1, 4, 9, 12, 13], 40)):
        want = pl.restate_planes(off, 8, rc.CLS, rc.SEP, 1, 0, False, [src[0][:ids_len]], [-1], ids_len=ids_len)
        assert want[4] == 8
        got = host_rows_planes(ht, ids, off, (8, rc.CLS, rc.SEP, 1, 0, False), src, [-1], len(want[1]), ids_len=ids_len)
        assert got[0] == len(want[1]) and got[3] == 8 and np.array_equal(got[1][0], want[0][0]), off


def host_span(ht, S, E, row_seq, nseq, first, last, none_cell, group=0):
    S = np.ascontiguousarray(S, dtype=np.int32); E = np.ascontiguousarray(E, dtype=np.int32)
    R, L = S.shape
    first = np.ascontiguousarray(first, dtype=np.int32); last = np.ascontiguousarray(last, dtype=np.int32)
    seq = None if row_seq is None else np.ascontiguousarray(row_seq, dtype=np.int32)
    s = np.full(R, CANARY32, dtype=np.int32); e = np.full(R, CANARY32, dtype=np.int32)
    st = ht.bft_span_rows(S.ctypes.data, E.ctypes.data, L, R, None if seq is None else seq.ctypes.data, nseq, first.ctypes.data, last.ctypes.data, none_cell,
                          s.ctypes.data, e.ctypes.data, group)
    return s, e, st


def test_b_span_groups(ht):
    """a wave for rows of more than 32 cells, the smallest power of two that covers the row below that"""
    assert [ht.bft_span_group(L) for L in (1, 2, 3, 4, 5, 8, 9, 16, 17, 31, 32, 33, 63, 64, 65, 130, 512, 1 << 20)] == [
        1, 2, 4, 4, 8, 8, 16, 16, 32, 32, 32, 64, 64, 64, 64, 64, 64, 64]


@pytest.mark.parametrize("L", [1, 5, 8, 31, 32, 33, 63, 64, 65, 130, 512])
def test_b_span_combine_on_random_planes(ht, L):
    """random planes in no order, a third of the cells without a token; spans of every kind; in the kernel's own partition and in every smaller
    and larger one (the result cannot depend on it)"""
    rnd = np.random.RandomState(L)
    R = 60
    S = rnd.randint(0, 40, size=(R, L)).astype(np.int32)
    S[rnd.rand(R, L) < 0.33] = -1
    S[0] = -1                                              # a row without any token
    E = (np.maximum(S, 0) + rnd.randint(0, 6, size=(R, L))).astype(np.int32)
    E[rnd.rand(R, L) < 0.1] = -3
    first = rnd.randint(-2, 45, size=R).astype(np.int32)
    last = (first + rnd.randint(-1, 8, size=R)).astype(np.int32)
    seq = rnd.randint(0, R, size=R).astype(np.int32)
    seq[3], seq[5] = R, -1                                 # two items out of range
    for row_seq, none in ((None, 0), (seq, -100)):
        want = pl.restate_span(S, E, row_seq, R, first, last, none)
        for group in (0, 1, 2, 16, 64):
            got = host_span(ht, S, E, row_seq, R, first, last, none, group)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2], (L, group)
    assert want[2] == 8 and (want[0] == -100).any() and (L < 5 or (want[0] != -100).any())      # (the inputs: spans found and not found)


def span_over_an_entry(ht, S, E, seq, nseq, first_token, none, loop_form):
    """answers of two whole tokens that begin at the first / second / third token of every item (token i = bytes 3 i .. 3 i + 1 of one numbering for
    the batch): the lane code equals the restatement; where an answer is found it is the cells of exactly those tokens"""
    for shift in (0, 1, 2):
        a = (3 * (np.asarray(first_token[:nseq], dtype=np.int64) + shift)).astype(np.int32)
        z = a + 4
        want = pl.restate_span_array(S, E, seq, nseq, a, z, none)
        if loop_form:                                                                   # (the array form of the restatement against the loop of the definition)
            loop = pl.restate_span(S, E, seq, nseq, a, z, none)
            assert np.array_equal(loop[0], want[0]) and np.array_equal(loop[1], want[1]) and loop[2] == want[2]
        got = host_span(ht, S, E, seq, nseq, a, z, none)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == 0, shift
        found = np.nonzero(want[0] != want[1])[0]
        assert (S[found, want[0][found]] == a[seq[found]]).all() and (E[found, want[1][found]] == z[seq[found]]).all() and (want[1][found] == want[0][found] + 1).all()
    return len(found)


@pytest.mark.parametrize("L", rc.TABLE_L)
def test_b_span_over_the_rows_table(ht, L):
    """monotone offsets through the planes of EVERY entry of the rows table with its synthetic input (every tenth entry also through the loop form)"""
    n = found = 0
    for par in rc.table():
        if par[0] != L:
            continue
        _, cls_id, sep_id, stride, max_rows, pad_left = par
        ids, off = rc.synthetic(*rc.geometry(L, cls_id, sep_id, stride), seed=n)
        starts = (3 * np.arange(len(ids))).astype(np.int32); ends = starts + 1
        (S, E), seq, _, _, _ = pl.restate_planes(off, L, cls_id, sep_id, stride, max_rows, pad_left, [starts, ends], [-1, -1])
        found += span_over_an_entry(ht, S, E, seq, len(off) - 1, off, -100 if pad_left else 0, n % 10 == 0)
        n += 1
    assert n == sum(1 for p in rc.table() if p[0] == L) and (L < 4 or found > 0)


@pytest.mark.parametrize("L", pc.TABLE_L)
def test_b_span_over_the_pairs_table(ht, L):
    """the same over EVERY entry of the pairs table: offsets over B alone, the fill over A"""
    n = found = 0
    for par in pc.table():
        if par[0] != L:
            continue
        _, cls_id, sep_id, double_sep, mode, max_a, stride, max_rows, pad_left = par
        srcs = pc.synthetic(par, seed=n)
        starts = (3 * np.arange(len(srcs[2]))).astype(np.int32); ends = starts + 1
        (S, E), seq, _, _, _ = pl.restate_pair_planes(srcs[1], srcs[3], L, cls_id, sep_id, mode, max_a, stride, max_rows, pad_left, double_sep, None, [starts, ends],
                                                      [-1, -1])
        found += span_over_an_entry(ht, S, E, seq, len(srcs[1]) - 1, srcs[3], -100 if pad_left else 0, n % 10 == 0)
        n += 1
    assert n == sum(1 for p in pc.table() if p[0] == L) and found > 0


def test_b_array_form_of_the_span_restatement_equals_the_loop():
    """random planes in no order, items out of range, a row count below the planes' rows: the array form the large cases use against the loop"""
    rnd = np.random.RandomState(2)
    for L, R in ((1, 5), (7, 40), (33, 60), (64, 30)):
        S = rnd.randint(0, 40, size=(R, L)).astype(np.int32); S[rnd.rand(R, L) < 0.33] = -1
        E = (np.maximum(S, 0) + rnd.randint(0, 6, size=(R, L))).astype(np.int32); E[rnd.rand(R, L) < 0.1] = -3
        first = rnd.randint(-2, 45, size=R).astype(np.int32); last = (first + rnd.randint(-1, 8, size=R)).astype(np.int32)
        seq = rnd.randint(-1, R + 1, size=R).astype(np.int32)
        for row_seq in (None, seq):
            for nrows in (None, 0, R - 2):
                a = pl.restate_span(S, E, row_seq, R, first, last, -100, nrows)
                b = pl.restate_span_array(S, E, row_seq, R, first, last, -100, nrows)
                assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2], (L, nrows)


# ---- (c) declared and exported
def test_c_new_symbols_are_declared_and_exported():
    import blingfire_amd as bf
    hdr = open(os.path.join(bfutil.ROOT, "include", "blingfiretokdll_amd.h")).read()
    exports = open(os.path.join(bfutil.ROOT, "blingfire_amd", "csrc", "exports.map")).read()
    lib = ctypes.CDLL(bf.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(r"BF_API\s+\w+\s+%s\(" % name, hdr), name
        assert re.search(r"^\s*%s;" % name, exports, flags=re.M), name
        assert hasattr(lib, name), name
    assert re.search(r"#define\s+BF_ROWS_MAX_PLANES\s+4\b", hdr)


def test_stand_alone_program_under_sanitizers(tmp_path):
    """the same file with its own main, built with -fsanitize=address,undefined and run as a program (never loaded into python)"""
    exe = str(tmp_path / "bf_planestest")
    src = os.path.join(bfutil.ROOT, "tests", "hosttest", "bf_planestest.cpp")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-DBF_PLANESTEST_MAIN", src, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("planes ok:"), r.stdout + r.stderr
