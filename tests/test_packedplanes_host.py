"""CPU tier of the companion planes of packed rows (IdsToPackedRowsPlanesBatch): the "where" lane code of blingfire_amd/csrc/bf_packed.h, compiled
for the host and driven in the lane partition of k_packed_planes at one and at four cells per lane (tests/hosttest/bf_packedplanestest.cpp), is
held to the restatement of packedplanes_cases on the parameter table, random batches, the exact-fit boundary, runs of width-0 units, bad ranges
and a truncated giant; packed_cell, which reads its ids through the same code, still gives the rows of packed_cases.restate; the restatement is
held to hand-made rows; the symbols are declared and exported; and the same unit runs once as a program of its own under ASan and UBSan."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import bfutil
import packed_cases as pc
import packedplanes_cases as pp

c_i64, c_int, c_vp = ctypes.c_int64, ctypes.c_int, ctypes.c_void_p
C, S, P = pc.CLS, pc.SEP, pc.PAD


@pytest.fixture(scope="module")
def ht():
    L = ctypes.CDLL(bfutil.HOSTTEST_LIB)
    L.bft_packedplanes_batch.restype = c_i64
    L.bft_packedplanes_batch.argtypes = [c_vp, c_i64, c_vp, c_i64, c_int, c_int, c_int, c_int, c_int, c_vp, c_vp, c_vp, c_vp, c_i64, c_int, c_vp]
    return L


def host_planes(ht, ids, off, L, cls, sep, src, fill, cap, lane_cells, ids_len=None, take=None):
    """-> (R, planes [cap, L] over canaries (None where not taken), rows [cap, L], status)"""
    ids = np.ascontiguousarray(ids, dtype=np.int32)
    off = np.ascontiguousarray(off, dtype=np.int64)
    src = [np.ascontiguousarray(s, dtype=np.int32) for s in src]
    n = len(src)
    take = [True] * n if take is None else take
    outs = [np.full((cap, L), pp.CANARY, dtype=np.int32) if t else None for t in take]
    rows = np.full((cap, L), pp.CANARY, dtype=np.int32)
    st = c_int(-1)
    c_src = (c_vp * max(n, 1))(*[s.ctypes.data for s in src])
    c_fill = (ctypes.c_int32 * max(n, 1))(*fill)
    c_out = (c_vp * max(n, 1))(*[None if o is None else o.ctypes.data for o in outs])
    R = ht.bft_packedplanes_batch(ids.ctypes.data, len(ids) if ids_len is None else ids_len, off.ctypes.data, len(off) - 1, L, cls, sep, P, n, c_src, c_fill, c_out,
                                  rows.ctypes.data, cap, lane_cells, ctypes.byref(st))
    return R, outs, rows, st.value


def check(ht, ids, off, L, cls, sep, nplanes=2, ids_len=None, what=None):
    n = len(ids) if ids_len is None else ids_len
    src = pp.sources(len(ids), nplanes, seed=L)
    fill = pp.FILLS[:nplanes]
    base = pc.restate(ids, off, L, cls, sep, P, ids_len=n)
    want = pp.restate_packed_planes(off, L, cls, sep, src, fill, ids_len=n)
    R = base[6]
    for lane_cells in (1, 4) if L % 4 == 0 else (1,):
        for cap in sorted({R, max(R - 1, 0), R + 2}):
            got_R, outs, rows, st = host_planes(ht, ids, off, L, cls, sep, src, fill, cap, lane_cells, ids_len=n)
            k = min(cap, R)
            assert got_R == R and st == (base[7] | (1 if R > cap else 0)), (what, L, cls, sep, lane_cells, cap)
            assert np.array_equal(rows[:k], base[0][:k]) and (rows[k:] == pp.CANARY).all(), (what, L, cls, sep, lane_cells, cap)
            for o, w in zip(outs, want):
                assert np.array_equal(o[:k], w[:k]) and (o[k:] == pp.CANARY).all(), (what, L, cls, sep, lane_cells, cap)
    return base, want


# ---- (a) the restatement itself, by hand
def test_a_the_restatement_on_hand_made_rows():
    off = [0, 2, 2, 7, 8]                                     # lengths 2, 0, 5, 1 at L = 6 with both specials: body 4
    src = [np.arange(10, 18, dtype=np.int32)]
    got = pp.restate_packed_planes(off, 6, C, S, src, [-1])[0]
    assert got.tolist() == [[-1, 10, 11, -1, -1, -1],         # [CLS] a b [SEP] [CLS] [SEP]
                            [-1, 12, 13, 14, 15, -1],         # the third sequence truncated to its first four ids: element 16 is not read
                            [-1, 17, -1, -1, -1, -1]]         # [CLS] h [SEP] and padding
    got = pp.restate_packed_planes(off, 6, -1, -1, src, [5])[0]
    assert got.tolist() == [[10, 11, 5, 5, 5, 5], [12, 13, 14, 15, 16, 17]]     # no specials: the empty sequence has no cell, padding takes the fill
    # a sequence outside [0, ids_len) is read as empty
    got = pp.restate_packed_planes([0, 2, 9], 4, -1, S, src, [0], ids_len=8)[0]
    assert got.tolist() == [[10, 11, 0, 0]]


# ---- (b) the lane code against the restatement
@pytest.mark.parametrize("L", pc.TABLE_L)
def test_b_parameter_table(ht, L):
    n = 0
    for l, cls, sep in pc.table():
        if l != L:
            continue
        ids, off = pc.synthetic(pc.geometry(L, cls, sep), seed=n)
        for nplanes in (1, 2, 4):
            check(ht, ids, off, L, cls, sep, nplanes, what="table")
        n += 1
    assert n > 0


@pytest.mark.parametrize("L,cls,sep", [(12, C, S), (7, -1, S), (8, -1, -1), (64, C, -1)])
def test_b_mixed_batches(ht, L, cls, sep):
    for seed in (1, 2, 3):
        ids, off = pc.mixed(300, seed, L, cls, sep)
        check(ht, ids, off, L, cls, sep, what=("mixed", seed))


@pytest.mark.parametrize("L", [8, 64])
def test_b_exact_fit(ht, L):
    ids, off = pc.exact_fit(L)
    check(ht, ids, off, L, -1, -1, what="exact fit")


def test_b_width_zero_runs(ht):
    ids, off = pc.ragged([3] + [0] * 20000 + [2])
    base, want = check(ht, ids, off, 8, -1, -1, nplanes=1, what="width 0")
    assert base[6] == 1 and (want[0][0] != pp.FILLS[0]).sum() == 5           # the two sequences share the row, 20000 units of width 0 between them
    check(ht, ids, off, 8, C, S, nplanes=1, what="specials only")


def test_b_bad_ranges(ht):
    ids = (1000 + np.arange(60)).astype(np.int32)
    for off, ids_len in pp.bad_range_cases():
        base, want = check(ht, ids, off, 8, C, S, ids_len=ids_len, what=("bad", off))
        assert base[7] == 8
        for q in range(len(off) - 1):
            if off[q] < 0 or off[q + 1] < off[q] or off[q + 1] > ids_len:         # read as empty: no id cells
                r, c = base[4][q], base[5][q]
                assert (want[0][r][c:c + 2] == pp.FILLS[0]).all()


def test_b_a_truncated_giant(ht):
    ids, off = pc.ragged([3, 0, 7, 50000, 1, 6, 9])
    src = pp.sources(len(ids), 1, seed=8)
    base, want = check(ht, ids, off, 8, C, S, nplanes=1, what="giant")
    r = base[4][3]
    assert want[0][r].tolist() == [-1] + src[0][10:16].tolist() + [-1]        # body 6: elements 10 .. 15 of the source, none of the 49994 behind them
    check(ht, ids, off, 64, -1, -1, what="giant")


def test_b_planes_not_taken(ht):
    ids, off = pc.mixed(60, 4, 8, C, S)
    src = pp.sources(len(ids), 3)
    want = pp.restate_packed_planes(off, 8, C, S, src, pp.FILLS[:3])
    R = want[0].shape[0]
    for take in ([True, False, True], [False, False, True], [False, False, False]):
        for cap in (R, R - 1):
            got_R, outs, _, st = host_planes(ht, ids, off, 8, C, S, src, pp.FILLS[:3], cap, 4, take=take)
            assert got_R == R and st == (1 if cap < R and any(take) else 0)   # no plane taken: nothing was dropped
            for o, w, t in zip(outs, want, take):
                assert (o is None) == (not t) and (o is None or np.array_equal(o, w[:cap]))


# ---- (c) declared and exported; the stand-alone program
def test_c_new_symbols_are_declared_and_exported():
    import blingfire_amd as bf
    hdr = open(os.path.join(bfutil.ROOT, "include", "blingfiretokdll_amd.h")).read()
    exports = open(os.path.join(bfutil.ROOT, "blingfire_amd", "csrc", "exports.map")).read()
    lib = ctypes.CDLL(bf.LIB_PATH)
    for name in ("IdsToPackedRowsPlanesBatchDevice", "IdsToPackedRowsPlanesBatch"):
        assert re.search(r"BF_API\s+\w+\s+%s\(" % name, hdr)
        assert re.search(r"^\s*%s;" % name, exports, flags=re.M)
        assert hasattr(lib, name)
    assert "have no companion planes" not in hdr and "a host-buffer form, offset planes of packed rows" not in hdr
    assert {"planes", "fill"} <= set(inspect.signature(bf.ids_to_packed_rows_batch_device).parameters)
    assert "return_offsets" in inspect.signature(bf.encode_packed_batch_device).parameters
    assert inspect.signature(bf.encode_packed_mlm_batch_device).parameters["whole_word"].default is True
    assert callable(bf.ids_to_packed_rows_planes_batch)


def test_stand_alone_program_under_sanitizers(tmp_path):
    """the lane-code driver with its own main, built with -fsanitize=address,undefined and run as a program (never loaded into python)"""
    exe = str(tmp_path / "bf_packedplanestest")
    src = os.path.join(bfutil.ROOT, "tests", "hosttest", "bf_packedplanestest.cpp")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-DBF_PACKEDPLANESTEST_MAIN", src, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("packedplanes ok:"), r.stdout + r.stderr
