"""The offsets call of a BPE model on the wave program, on the host (tests/hosttest/bf_bpeoffstest.cpp): the SPANS instance of BpeWave in the wave
simulator, the handed-back documents through BpeSeg with spans, then the per-block span logic k_bpe_home_spans shares with the unit
(blingfire_amd/csrc/bf_bpe_home.h) -- count, ids, first byte and last byte of every document of the unit's case table against the oracle, for max_ids
above the token counts, 3 and 1.  A handed-back document and an end taken from the look-ahead mask must each have occurred; with gpt2.bin also a
word of solve_big and one of unit_huge.  The same unit as a stand-alone program runs once under the address and undefined-behaviour sanitizers
(blingfire_amd/build.py build_bpeoffs_san)."""
import ctypes
import os
import subprocess

import pytest

import bfutil

MODELS = [m for m in ("gpt2.bin", "roberta.bin", "bpe_example.bin", "bpe_example2.bin") if bfutil.have_model(m)]


@pytest.mark.parametrize("model", MODELS)
def test_case_table_against_the_oracle(model):
    L = ctypes.CDLL(bfutil.HOSTTEST_LIB)
    L.bft_bpeoffs_run.restype = ctypes.c_long
    L.bft_bpeoffs_run.argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_ulonglong)]
    reached = (ctypes.c_ulonglong * 4)()
    diffs = L.bft_bpeoffs_run(bfutil.model_path(model).encode(), reached)
    back, ahead, big, huge = list(reached)
    assert diffs == 0 and back > 0 and ahead > 0, (model, diffs, back, ahead)
    assert model != "gpt2.bin" or (big > 0 and huge > 0), (big, huge)


def test_stand_alone_program_under_the_sanitizers(tmp_path):
    from blingfire_amd import build
    exe = build.build_bpeoffs_san(str(tmp_path))
    env = dict(os.environ, ASAN_OPTIONS="abort_on_error=0:detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe] + [bfutil.model_path(m) for m in MODELS[:1]], capture_output=True, text=True, errors="replace", timeout=600, env=env)
    assert r.returncode == 0 and "ERROR: AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr, (r.returncode, r.stderr[-2000:], r.stdout[-400:])
