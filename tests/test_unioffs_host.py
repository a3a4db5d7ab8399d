"""The offsets instance of the Unigram cut form on the host (tests/hosttest/bf_unioffstest.cpp): bf_seg.h UniCut with span words in the host
driver's trip, then what k_uni_ids makes of them, against the oracle's (id, first byte, last byte) on the unit's case table -- dummy prefix on
and off, max_ids above and below the token count, four driver shapes -- and, for the restart that no shipped model reaches, against the
sequential restatement on a dictionary with a positive score.  The restart, a spill and the short way out must each have been taken.  The same
unit as a stand-alone program runs once under the address and undefined-behaviour sanitizers (blingfire_amd/build.py build_unioffs_san)."""
import ctypes
import os
import subprocess

import pytest

import bfutil

MODELS = [m for m in ("xlm_roberta_base.bin", "xlnet.bin", "laser500k.bin") if bfutil.have_model(m)]


@pytest.fixture(scope="module")
def run():
    L = ctypes.CDLL(bfutil.HOSTTEST_LIB)
    L.bft_unioffs_run.restype = ctypes.c_long
    L.bft_unioffs_run.argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_ulonglong)]

    def call(path):
        reached = (ctypes.c_ulonglong * 3)()
        return L.bft_unioffs_run(path, reached), list(reached)
    return call


def test_restart_against_the_sequential_form(run):
    diffs, (restarts, _, quick) = run(None)
    assert diffs == 0 and restarts > 0 and quick > 0, (diffs, restarts, quick)


@pytest.mark.parametrize("model", MODELS)
def test_case_table_against_the_oracle(run, model):
    diffs, (_, spills, quick) = run(bfutil.model_path(model).encode())
    assert diffs == 0 and spills > 0 and quick > 0, (model, diffs, spills, quick)


def test_stand_alone_program_under_the_sanitizers(tmp_path):
    from blingfire_amd import build
    exe = build.build_unioffs_san(str(tmp_path))
    env = dict(os.environ, ASAN_OPTIONS="abort_on_error=0:detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe] + [bfutil.model_path(m) for m in MODELS[:1]], capture_output=True, text=True, errors="replace", timeout=600, env=env)
    assert r.returncode == 0 and "ERROR: AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr, (r.returncode, r.stderr[-2000:], r.stdout[-400:])
