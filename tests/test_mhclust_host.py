"""CPU tier of the MinHash clusters (MinHashClustersBatchDevice): the symbol is declared, exported, in the signature table and refuses a call
without a handle; what the two wrappers send to the library, against the recording stand-in of test_wrapper_calls.py; the lane code of
blingfire_amd/csrc/bf_mhclust.h, compiled for the host and run sequentially in both visiting orders (tests/hosttest/bf_mhclusttest.cpp), against
the restatement of mhclust_cases; and the same unit once as a program of its own under ASan and UBSan."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import bfutil
import mhclust_cases as cc
from test_wrapper_calls import P, N, dev_docs, env, shapes  # noqa: F401  (env is the fixture)

NAME = "MinHashClustersBatchDevice"
c_i64, c_int, c_vp = ctypes.c_int64, ctypes.c_int, ctypes.c_void_p


def test_symbol_is_declared_exported_and_refuses_a_null_handle():
    import blingfire_amd as bf
    hdr = open(os.path.join(bfutil.ROOT, "include", "blingfiretokdll_amd.h")).read()
    exports = open(os.path.join(bfutil.ROOT, "blingfire_amd", "csrc", "exports.map")).read()
    assert re.search(r"BF_API\s+\w+\s+%s\(" % NAME, hdr) and re.search(r"^\s*%s;" % NAME, exports, flags=re.M)
    assert NAME in bf._SIGNATURES and len(bf._SIGNATURES[NAME][1]) == 14
    assert NAME in hdr[hdr.index("Status word of the last batch call"):hdr.index("BF_API int BfLastStatus")]
    assert getattr(ctypes.CDLL(bf.LIB_PATH), NAME)(*[None] * 14) == -1           # refused without a device
    assert "bf_kernels_mhclust.hip" in open(os.path.join(bfutil.ROOT, "blingfire_amd", "build.py")).read()


def test_wrapper_calls(env):
    bf, L, torch = env.bf, env.L, env.torch
    keys, sig, nsh = torch.zeros((3, 4), dtype=torch.int64), torch.zeros((3, 32), dtype=torch.int32), torch.ones(3, dtype=torch.int32)
    outs = [((3,), "int32"), ((3,), "bool"), ((3,), "int32"), ((2,), "int64")]
    assert shapes(bf.minhash_clusters_device(7, keys, stream=9)) == outs
    assert shapes(bf.minhash_clusters_device(7, keys, sig, 20, nsh)) == outs
    got = bf.encode_dedup_batch_device(7, *dev_docs(torch), 6, num_perm=64, shingle=2, band_rows=8, min_jaccard=0.8, seed=3, unk=5)
    assert shapes(got) == [((2,), "int32"), ((2,), "bool"), ((2,), "int32"), ((2,), "int64"), ((2, 64), "int32"), ((2,), "int32")]
    assert [e for e in L.log if e[0] != "BfLastError"] == [
        (NAME, (P, N, 1, P, 4, 3, N, 0, 0, P, P, P, P, P)), (NAME, (P, P, 32, P, 4, 3, P, 20, 0, P, P, P, P, P)),
        ("TextToIdsBatchDevice", (P, P, P, 2, 3, P, 10, P, 6, 5, P)), ("IdsToMinHashBatchDevice", (P, P, 10, P, 2, 2, 64, 8, 3, 0, P, 2, P, P, P)),
        (NAME, (P, P, 64, P, 8, 2, P, 52, 0, P, P, P, P, P))]                     # ceil(0.8 * 64) = 52
    assert env.streams                                          # without `stream`: torch's current stream


@pytest.fixture(scope="module")
def ht():
    L = ctypes.CDLL(bfutil.HOSTTEST_LIB)
    L.bft_mhclust_batch.restype = c_int
    L.bft_mhclust_batch.argtypes = [c_vp, c_int, c_vp, c_int, c_i64, c_vp, c_int, c_int] + [c_vp] * 5
    g = (c_i64 * 3)()
    L.bft_mhclust_geometry(g)
    assert g[0] == cc.EMPTY and g[1] == 2064 and 0 <= g[2] < 2063
    return L


def check_host(ht, keys, sig, min_equal, nsh, want):
    nseq, B = keys.shape
    for reverse in (0, 1):
        label, keep, size = np.full(nseq, -7, np.int32), np.full(nseq, 7, np.uint8), np.full(nseq, -7, np.int32)
        counts, info = np.zeros(2, np.int64), np.zeros(1, np.int64)
        assert ht.bft_mhclust_batch(None if sig is None else sig.ctypes.data, 1 if sig is None else sig.shape[1], keys.ctypes.data, B, nseq,
                                    None if nsh is None else nsh.ctypes.data, min_equal, reverse, *(a.ctypes.data for a in (label, keep, size, counts, info))) == 0
        for name, g in zip(("label", "keep", "size", "counts"), (label, keep, size, counts)):
            assert np.array_equal(g, want[name]), (name, reverse)


@pytest.mark.parametrize("nseq,B,H,min_equal", cc.table())
def test_lane_code_random_table(ht, nseq, B, H, min_equal):
    keys, sig, nsh, want = cc.random_case(nseq, B, H, min_equal)
    check_host(ht, keys, sig, min_equal, nsh, want)


@pytest.mark.parametrize("name", cc.NAMED)
def test_lane_code_named_shapes(ht, name):
    keys, says = cc.named(name)
    want = cc.restate(keys)
    assert want["counts"].tolist() == [says["clusters"], says["candidates"]]
    check_host(ht, keys, None, 0, None, want)


def test_stand_alone_program_under_sanitizers(tmp_path):
    """the lane-code driver with its own main, built with -fsanitize=address,undefined and run as a program (never loaded into python)"""
    exe = str(tmp_path / "bf_mhclusttest")
    src = os.path.join(bfutil.ROOT, "tests", "hosttest", "bf_mhclusttest.cpp")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-DBF_MHCLUSTTEST_MAIN", src, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("mhclust ok:"), r.stdout + r.stderr
