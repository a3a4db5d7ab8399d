"""CPU tier of the n-gram calls (IdsToNgramSetBatchDevice, IdsNgramOverlapBatchDevice): the two names are declared, exported, in the signature table
and refuse a call without a handle; what the four wrappers send to the library, against the recording stand-in of test_wrapper_calls.py; the lane
code of blingfire_amd/csrc/bf_ngram.h, compiled for the host and run sequentially in the kernel's partition (tests/hosttest/bf_ngramtest.cpp),
against the restatement of ngram_cases over its case table; and the same unit once as a program of its own under ASan and UBSan."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import bfutil
import ngram_cases as nc
from test_wrapper_calls import P, N, dev_docs, dev_ragged, env, raises, shapes  # noqa: F401  (env is the fixture)

SET, OVER = "IdsToNgramSetBatchDevice", "IdsNgramOverlapBatchDevice"
vp = ctypes.c_void_p


def test_symbols_are_declared_exported_and_refuse_a_null_handle():
    import blingfire_amd as bf
    hdr = open(os.path.join(bfutil.ROOT, "include", "blingfiretokdll_amd.h")).read()
    exports = open(os.path.join(bfutil.ROOT, "blingfire_amd", "csrc", "exports.map")).read()
    for name, nargs in ((SET, 12), (OVER, 15)):
        assert re.search(r"BF_API\s+\w+\s+%s\(" % name, hdr) and re.search(r"^\s*%s;" % name, exports, flags=re.M)
        assert name in bf._SIGNATURES and len(bf._SIGNATURES[name][1]) == nargs
        assert getattr(ctypes.CDLL(bf.LIB_PATH), name)(*[None] * nargs) == -1    # refused without a device


def test_wrapper_calls(env):
    bf, L, torch = env.bf, env.L, env.torch
    d_ids, d_off = dev_ragged(torch)
    table, counts = bf.ngram_set_device(7, d_ids, d_off, stream=9)              # allocates 2 * 3 + 64 slots and clears them
    assert shapes((table, counts)) == [((70,), "int64"), ((3,), "int64")]
    assert bf.ngram_set_device(7, d_ids, d_off, 8, -1, table)[0] is table      # a table given is added to
    assert shapes(bf.ngram_set_device(7, d_ids, d_off, 8, 5, table, clear=True, stream=9)) == shapes((table, counts))
    assert shapes(bf.ngram_set_device(7, d_ids, d_off, slots=9, stream=9)) == [((9,), "int64"), ((3,), "int64")]
    raises(ValueError, "table must be a contiguous torch.int64 tensor of at least 2 slots on cpu", bf.ngram_set_device, 7, d_ids, d_off, table=table[:1])
    assert shapes(bf.ngram_overlap_device(7, d_ids, d_off, table, stream=9)) == [((2,), "int32")] * 3
    assert shapes(bf.ngram_overlap_device(7, d_ids, d_off, table, 8, 5, True)) == [((2,), "int32")] * 3 + [((3,), "bool")]
    assert shapes(bf.encode_ngram_set_batch_device(7, *dev_docs(torch), 6, n=4, seed=3, unk=5)) == [((84,), "int64"), ((3,), "int64")]
    got = bf.encode_ngram_overlap_batch_device(7, *dev_docs(torch), 6, table, n=4, seed=3, return_mask=True, unk=5)
    assert shapes(got) == [((2,), "int32")] * 3 + [((10,), "bool"), ((10,), "int32"), ((3,), "int64")]
    L.script[OVER] = -2
    raises(RuntimeError, OVER + " failed (-2): boom", bf.ngram_overlap_device, 7, d_ids, d_off, table, stream=9)
    ids10 = ("TextToIdsBatchDevice", (P, P, P, 2, 3, P, 10, P, 6, 5, P))
    assert [e for e in L.log if e[0] != "BfLastError"] == [
        (SET, (P, P, 3, P, 2, 13, 0, 1, P, 70, P, P)), (SET, (P, P, 3, P, 2, 8, (1 << 64) - 1, 0, P, 70, P, P)), (SET, (P, P, 3, P, 2, 8, 5, 1, P, 70, P, P)),
        (SET, (P, P, 3, P, 2, 13, 0, 1, P, 9, P, P)), (OVER, (P, P, 3, P, 2, 13, 0, 0, P, 70, P, P, P, N, P)), (OVER, (P, P, 3, P, 2, 8, 5, 0, P, 70, P, P, P, P, P)),
        ids10, (SET, (P, P, 10, P, 2, 4, 3, 1, P, 84, P, P)), ids10, (OVER, (P, P, 10, P, 2, 4, 3, 0, P, 70, P, P, P, P, P)),
        (OVER, (P, P, 3, P, 2, 13, 0, 0, P, 70, P, P, P, N, P))]


@pytest.fixture(scope="module")
def ht():
    L = ctypes.CDLL(bfutil.HOSTTEST_LIB)
    L.bft_ngram_batch.argtypes = [vp, ctypes.c_int64, vp, ctypes.c_int64, ctypes.c_int, ctypes.c_uint64, ctypes.c_int, vp, ctypes.c_int64] + [vp] * 5
    assert L.bft_ngram_facts() == 0       # the roll equals Horner for every n; fingerprint 0 is read as 1; a full table ends insert and look-up
    return L


@pytest.mark.parametrize("n", nc.NS)
def test_lane_code_over_the_case_table(ht, n):
    ids, off, s_ids, s_off = nc.case(n)
    members, want_counts = nc.build(s_ids, s_off, n, 5)
    want = nc.overlap(ids, off, n, 5, members)
    table, counts = np.full(len(members) + 1, 7, np.uint64), np.zeros(3, np.int64)           # one slot to spare: the probes wrap around the end
    a = lambda x: x.ctypes.data
    assert ht.bft_ngram_batch(a(s_ids), len(s_ids), a(s_off), len(s_off) - 1, n, 5, 3, a(table), len(table), a(counts), None, None, None, None) == 0
    assert counts.tolist() == want_counts.tolist() and set(table.tolist()) - {0} == members
    got = dict(ngrams=np.full(len(off) - 1, -7, np.int32), hits=np.full(len(off) - 1, -7, np.int32), covered=np.full(len(off) - 1, -7, np.int32), mask=np.full(len(ids), 7, np.uint8))
    assert ht.bft_ngram_batch(a(ids), len(ids), a(off), len(off) - 1, n, 5, 0, a(table), len(table), None, *(a(got[k]) for k in ("ngrams", "hits", "covered", "mask"))) == 8
    for k, g in got.items():
        assert np.array_equal(g, want[k]), k
    assert want["hits"].sum() > 0 and (want["hits"] < want["ngrams"]).any()


def test_stand_alone_program_under_sanitizers(tmp_path):
    """the lane-code driver with its own main, built with -fsanitize=address,undefined and run as a program (never loaded into python)"""
    exe = str(tmp_path / "bf_ngramtest")
    src = os.path.join(bfutil.ROOT, "tests", "hosttest", "bf_ngramtest.cpp")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-DBF_NGRAMTEST_MAIN", src, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("ngram ok:"), r.stdout + r.stderr
