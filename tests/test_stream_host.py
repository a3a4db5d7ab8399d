"""CPU tier of the stream rows (IdsToStreamRowsBatch): the lane code of blingfire_amd/csrc/bf_stream.h, compiled for the host and driven in the
tile partition of k_stream_fill at one and at four cells per lane, through the staged slice and through the search of W itself
(tests/hosttest/bf_streamtest.cpp), is held to the sequential restatement of stream_cases on the parameter table, the generators of
packed_cases, and tile cases built from the kernel's own tile constants; the restatement is held to the header's worked example by hand and the
vectorised restatement to the sequential one; the symbols are declared and exported; and the same unit runs once as a program of its own under
ASan and UBSan."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import bfutil
import packed_cases as pc
import stream_cases as sc

c_i64, c_int, c_vp = ctypes.c_int64, ctypes.c_int, ctypes.c_void_p
B, E, P, IGN = sc.BOS, sc.EOS, sc.PAD, sc.IGN


@pytest.fixture(scope="module")
def ht():
    L = ctypes.CDLL(bfutil.HOSTTEST_LIB)
    L.bft_stream_batch.restype = c_i64
    L.bft_stream_batch.argtypes = [c_vp, c_i64, c_vp, c_i64] + [c_int] * 6 + [c_vp] * 6 + [c_i64, c_vp, c_vp, c_vp, c_int, c_int, c_vp, c_vp]
    L.bft_stream_geometry.restype = None
    L.bft_stream_geometry.argtypes = [c_vp]
    return L


@pytest.fixture(scope="module")
def geo(ht):
    g = (c_int * 4)()
    ht.bft_stream_geometry(g)
    lanes, wide, stage, probes = list(g)
    assert lanes % 64 == 0 and wide == 4 and stage >= 64 and probes == 64
    return {"lanes": lanes, "wide": wide, "stage": stage}


def host_stream(ht, ids, off, L, bos, eos, flags, cap, lane_cells, force_global=0, ids_len=None, take=(True,) * 8):
    """-> (R, T, the eight outputs over canaries (None where not taken), status, [tiles staged, tiles searched in W, rounds of the longest search])"""
    ids = np.ascontiguousarray(ids, dtype=np.int32)
    off = np.ascontiguousarray(off, dtype=np.int64)
    nseq = len(off) - 1
    shapes = [(cap, L)] * 4 + [(cap,)] * 2 + [(nseq,)] * 2
    outs = [np.full(s, sc.CANARY, dtype=np.int32) if t else None for s, t in zip(shapes, take)]
    nrows = np.full(2, -1, dtype=np.int64)
    info = np.zeros(3, dtype=np.int64)
    st = c_int(-1)
    a = [None if o is None else o.ctypes.data for o in outs]
    R = ht.bft_stream_batch(ids.ctypes.data, len(ids) if ids_len is None else ids_len, off.ctypes.data, nseq, L, bos, eos, P, IGN, flags, *a[:6], cap, *a[6:],
                            nrows.ctypes.data, lane_cells, force_global, info.ctypes.data, ctypes.byref(st))
    assert R < 0 or nrows.tolist()[0] == R
    return R, int(nrows[1]), outs, st.value, info.tolist()


def check(ht, ids, off, L, bos, eos, flags, ids_len=None, what=None, caps=None, want=None):
    """both lane forms and both paths, at several capacities, against the sequential restatement; -> (the restatement, info of the auto path at cap R)"""
    n = len(ids) if ids_len is None else ids_len
    if want is None:
        want = sc.restate(ids, off, L, bos, eos, P, IGN, flags, ids_len=n)
    R, T = want[8], want[9]
    info_at_R = None
    for lane_cells in (1, 4) if L % 4 == 0 else (1,):
        for force in (0, 1):
            for cap in sorted({R, max(R - 1, 0), R + 2}) if caps is None else caps:
                key = (what, L, bos, eos, flags, lane_cells, force, cap)
                got_R, got_T, outs, st, info = host_stream(ht, ids, off, L, bos, eos, flags, cap, lane_cells, force, ids_len=n)
                k = min(cap, R)
                assert (got_R, got_T) == (R, T) and st == (want[10] | (1 if R > cap else 0)), key
                for i, (o, w) in enumerate(zip(outs, want[:8])):
                    kk = k if i < 6 else len(w)
                    assert np.array_equal(o[:kk], w[:kk]) and (o[kk:] == sc.CANARY).all(), (key, sc.NAMES[i])
                assert info[2] <= 6 and (force == 0 or info[0] == 0), key
                if cap == R and force == 0 and lane_cells == (4 if L % 4 == 0 else 1):
                    info_at_R = info
    return want, info_at_R


# ---- (a) the restatements themselves
def test_a_the_worked_example_by_hand():
    ids = np.arange(1000, 1010, dtype=np.int32)
    w = sc.restate(ids, [0, 3, 3, 3, 10], 4, 1, 2, 0, -100, 0)
    assert (w[8], w[9], w[10]) == (5, 18, 0)
    assert w[0].tolist() == [[1, 1000, 1001, 1002], [2, 1, 2, 1], [2, 1, 1003, 1004], [1005, 1006, 1007, 1008], [1009, 2, 0, 0]]
    assert w[1].tolist() == [[1, 1, 1, 1], [1, 2, 2, 3], [1, 2, 2, 2], [1, 1, 1, 1], [1, 1, 0, 0]]
    assert w[2].tolist() == [[0, 1, 2, 3], [4, 0, 1, 0], [1, 0, 1, 2], [3, 4, 5, 6], [7, 8, 0, 0]]
    assert w[3].tolist() == [[1000, 1001, 1002, 2], [1, 2, 1, 2], [1, 1003, 1004, 1005], [1006, 1007, 1008, 1009], [2, -100, -100, -100]]
    assert w[4].tolist() == [0, 0, 2, 3, 3] and w[5].tolist() == [0, 4, 1, 3, 7]
    assert w[6].tolist() == [0, 1, 1, 2] and w[7].tolist() == [0, 1, 3, 1]
    # flags: drop the last row (its label at the edge still comes from the stream); positions from the row's edge; labels inside a unit only
    d = sc.restate(ids, [0, 3, 3, 3, 10], 4, 1, 2, 0, -100, sc.DROP_LAST)
    assert d[8] == 4 and np.array_equal(d[0], w[0][:4]) and d[3][3].tolist() == [1006, 1007, 1008, 1009] and d[6].tolist() == [0, 1, 1, 2]
    e = sc.restate(ids, [0, 3, 3, 3, 10], 4, 1, 2, 0, -100, sc.POS_FROM_ROW)
    assert e[2].tolist() == [[0, 1, 2, 3], [0, 0, 1, 0], [0, 0, 1, 2], [0, 1, 2, 3], [0, 1, 0, 0]]
    g = sc.restate(ids, [0, 3, 3, 3, 10], 4, 1, 2, 0, -100, sc.LABELS_WITHIN)
    assert g[3].tolist() == [[1000, 1001, 1002, 2], [-100, 2, -100, 2], [-100, 1003, 1004, 1005], [1006, 1007, 1008, 1009], [2, -100, -100, -100]]
    # no specials: units of width 0 are counted by seg and have a cell of their own in seq_row / seq_col
    z = sc.restate(ids, [0, 3, 3, 3, 10], 4)
    assert (z[8], z[9]) == (3, 10) and z[1].tolist() == [[1, 1, 1, 4], [1, 1, 1, 1], [1, 1, 0, 0]] and z[6].tolist() == [0, 0, 0, 0] and z[7].tolist() == [0, 3, 3, 3]
    # nothing at all, and units of width 0 only: no row
    assert sc.restate([], [0], 4, 1, 2)[8:] == (0, 0, 0) and sc.restate([], [0, 0, 0], 4)[8:] == (0, 0, 0)
    # a sequence outside [0, ids_len] is read as empty
    b = sc.restate(ids, [0, 2, 12], 4, -1, 2, ids_len=10)
    assert b[0].tolist() == [[1000, 1001, 2, 2]] and b[10] == 8


@pytest.mark.parametrize("L", sc.TABLE_L)
def test_a_vectorised_restatement_equals_the_sequential_one(L):
    for (l, bos, eos, flags) in sc.table():
        if l != L:
            continue
        ids, off = pc.mixed(120, L + flags, max(L, 4))
        assert sc.same(sc.restate(ids, off, L, bos, eos, P, IGN, flags), sc.restate_np(ids, off, L, bos, eos, P, IGN, flags)), (L, bos, eos, flags)
    ids = (1000 + np.arange(60)).astype(np.int32)
    for off, ids_len in (([0, 5, 3, 12, 20], 60), ([0, 10, 70, 70, 80], 60), ([0, 10, 20, 35, 60], 30), ([-1, 4, 9], 60), ([0], 0), ([0, 0, 0], 0)):
        assert sc.same(sc.restate(ids, off, L, B, E, ids_len=ids_len), sc.restate_np(ids, off, L, B, E, ids_len=ids_len))
        assert sc.same(sc.restate(ids, off, L, ids_len=ids_len), sc.restate_np(ids, off, L, ids_len=ids_len))


# ---- (b) the lane code against the sequential restatement
@pytest.mark.parametrize("L", sc.TABLE_L)
def test_b_parameter_table(ht, L):
    n = 0
    for (l, bos, eos, flags) in sc.table():
        if l != L:
            continue
        ids, off = sc.ragged([0, 1, L - 1, L, L + 1, 3 * L, 0, 0, 2, 7 * L + 3, 1, 1, 0], seed=n)
        check(ht, ids, off, L, bos, eos, flags, what="table")
        ids, off = pc.mixed(150, n, max(L, 4))                 # (the generator's lengths are drawn for a row of at least 4 cells)
        check(ht, ids, off, L, bos, eos, flags, what="mixed")
        n += 1
    assert n == 32


@pytest.mark.parametrize("L", [4, 5, 8, 64])
def test_b_exact_fit_and_ragged(ht, L):
    for flags in (0, 7):
        if L >= 4:
            ids, off = pc.exact_fit(max(L, 4))
            check(ht, ids, off, L, -1, -1, flags, what="exact fit")
            check(ht, ids, off, L, B, E, flags, what="exact fit")
        ids, off = pc.ragged([3, 0, 7, 5000, 1, 6, 9])
        check(ht, ids, off, L, B, E, flags, what="ragged")
        check(ht, ids, off, L, -1, E, flags, what="ragged")


def test_b_bad_ranges(ht):
    ids = (1000 + np.arange(60)).astype(np.int32)
    for off, ids_len in (([0, 5, 3, 12, 20], 60), ([0, 10, 70, 70, 80], 60), ([0, 10, 20, 35, 60], 30), ([-1, 4, 9], 60)):
        for L, bos, eos in ((8, B, E), (5, -1, -1), (4, -1, E)):
            want, _ = check(ht, ids, off, L, bos, eos, 0, ids_len=ids_len, what=("bad", off))
            assert want[10] == 8


def test_b_nothing_to_cut(ht):
    for off in ([0], [0, 0, 0, 0]):
        want, _ = check(ht, [], off, 4, -1, -1, 0, what="T = 0")
        assert want[8:] == (0, 0, 0)
        want, _ = check(ht, [], off, 4, B, E, 1, what="specials only")
        assert want[9] == 2 * (len(off) - 1)
    for T in (1, 3, 4, 5):                                       # T around L, with and without the dropped tail
        ids, off = sc.ragged([T])
        for flags in (0, 1):
            want, _ = check(ht, ids, off, 4, -1, -1, flags, what=("T", T))
            assert want[8] == (T // 4 if flags else -(-T // 4))


# ---- (c) the tile: cases built from the kernel's own constants
@pytest.mark.parametrize("wide", [True, False])
def test_c_tile_cases(ht, geo, wide):
    tc, su = geo["lanes"] * (geo["wide"] if wide else 1), geo["stage"]
    seen = {}
    for name, lens, L, bos, eos in sc.tile_cases(tc, su, wide):
        assert (L % 4 == 0) == wide
        ids, off = sc.ragged(lens)
        want = sc.restate_np(ids, off, L, bos, eos, P, IGN, 0)
        if len(lens) < 3000:
            assert sc.same(want, sc.restate(ids, off, L, bos, eos, P, IGN, 0)), name
        R = want[8]
        _, info = check(ht, ids, off, L, bos, eos, 0, what=name, caps=[R, max(R - 1, 0)], want=want)
        check(ht, ids, off, L, bos, eos, 7, what=name, caps=[R])
        seen[name] = info
    # the staged capacity: a slice of capacity - 1 and of exactly the capacity is staged, one unit more is searched in W itself
    for kind in ("staged", "zeros"):
        assert seen[kind + "-1"][1] == 0 and seen[kind + "+0"][1] == 0 and seen[kind + "+1"][1] == 1, (kind, seen)
    # a run of units of width 0 inside the stream is part of a tile's slice; one at the very start or the very end of the stream is part of none
    # (a cell's unit is the LAST one that begins at or in front of it, and the units behind the last cell begin at T)
    assert seen["zero-run"][1] >= 1 and seen["zero-run-start-end"][1] == 0 and seen["zero-run-start-end-long"][1] == 0
    assert seen["three-tiles"][0] >= 4 and seen["three-tiles"][1] == 0
    assert seen["long-row"][0] >= 5 and seen["long-row"][1] == 0


def test_c_search_rounds(ht):
    """the search of the whole W shrinks its range 64-fold a round: two rounds for up to 64 * 64 units, three beyond"""
    for nseq, rounds in ((1, 0), (2, 1), (64, 1), (65, 2), (4096, 2), (4097, 3)):
        ids, off = sc.ragged([1] * nseq)
        _, _, _, _, info = host_stream(ht, ids, off, 4, -1, -1, 0, nseq, 4)
        assert info[2] == rounds, (nseq, info)


def test_c_outputs_not_taken(ht):
    ids, off = pc.mixed(60, 4, 8)
    want = sc.restate(ids, off, 8, B, E, P, IGN, 0)
    R = want[8]
    for take in ([True] * 8, [False] * 8, [False, True, False, True, False, True, False, True], [False] * 4 + [True, False, True, False], [False] * 6 + [True] * 2):
        for cap in (R, R - 1):
            got_R, _, outs, st, _ = host_stream(ht, ids, off, 8, B, E, 0, cap, 4, take=take)
            assert got_R == R and st == (1 if cap < R and any(take[:6]) else 0)
            for i, (o, w, t) in enumerate(zip(outs, want[:8], take)):
                n = cap if i < 6 else len(w)                   # the per-sequence outputs are complete whatever the capacity is
                assert (o is None) == (not t) and (o is None or np.array_equal(o[:n], w[:n]))


# ---- (d) declared and exported; the stand-alone program
def test_d_new_symbols_are_declared_and_exported():
    import blingfire_amd as bf
    hdr = open(os.path.join(bfutil.ROOT, "include", "blingfiretokdll_amd.h")).read()
    exports = open(os.path.join(bfutil.ROOT, "blingfire_amd", "csrc", "exports.map")).read()
    lib = ctypes.CDLL(bf.LIB_PATH)
    for name in ("IdsToStreamRowsBatchDevice", "IdsToStreamRowsBatch"):
        assert re.search(r"BF_API\s+\w+\s+%s\(" % name, hdr)
        assert re.search(r"^\s*%s;" % name, exports, flags=re.M)
        assert hasattr(lib, name)
    assert "After IdsToStreamRowsBatchDevice" in hdr
    p = inspect.signature(bf.encode_clm_batch_device).parameters
    assert [p[k].default for k in ("unk", "ignore_label", "drop_last", "pos_from_row", "labels_within_doc", "rows_cap")] == [0, -100, False, False, False, None]
    assert "max_ids_per_doc" in p and "rows_cap" in inspect.signature(bf.ids_to_stream_rows_batch_device).parameters
    assert callable(bf.ids_to_stream_rows_batch) and callable(bf.encode_clm_batch)


def test_stand_alone_program_under_sanitizers(tmp_path):
    """the lane-code driver with its own main, built with -fsanitize=address,undefined and run as a program (never loaded into python)"""
    exe = str(tmp_path / "bf_streamtest")
    src = os.path.join(bfutil.ROOT, "tests", "hosttest", "bf_streamtest.cpp")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-DBF_STREAMTEST_MAIN", src, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("stream ok:"), r.stdout + r.stderr
