"""CPU tier of MinHash (IdsToMinHashBatchDevice): the restatement of minhash_cases estimates the Jaccard similarity of shingle sets within the
estimator's own standard deviation; its numpy minimum equals Python ints; the new symbols are declared, exported, in the signature table and
refuse a call without a handle before they touch a device."""
import ctypes
import math
import os
import re

import numpy as np

import bfutil
import minhash_cases as mc


def test_equal_slots_estimate_the_jaccard_similarity():
    rng = np.random.default_rng(3)
    k, H, err = 3, 256, []
    for pair in range(40):
        a = rng.integers(0, 30000, size=300).astype(np.int32)
        b = a.copy()
        at = rng.choice(300, size=int(rng.integers(0, 61)), replace=False)
        b[at] = rng.integers(30000, 60000, size=len(at))
        sa, sb = ({tuple(s) for s in mc.shingles(x.tolist(), k)} for x in (a, b))
        sig = mc.restate(np.concatenate([a, b]), np.array([0, 300, 600]), k, H, seed=pair)["sig"]
        err.append(abs(float((sig[0] == sig[1]).mean()) - len(sa & sb) / len(sa | sb)))
    assert sum(err) / len(err) < 2 * math.sqrt(0.25 / H), err


def test_numpy_minimum_equals_python_ints():
    seed = mc.M64
    ids, off = mc.ragged([0, 1, 4, 5, 9], 5)
    want = mc.restate(ids, off, 5, 65, seed=seed)["sig"].view(np.uint32)
    for q in range(5):
        hs = [mc.shingle_hash(s, seed) for s in mc.shingles(ids[off[q]:off[q + 1]].tolist(), 5)]
        for i, (a, b) in enumerate(mc.perm(seed, i) for i in range(65)):
            assert a & 1 and want[q, i] == min([((a * s + b) & mc.M64) >> 32 for s in hs], default=mc.EMPTY)


def test_new_symbols_are_declared_exported_and_refuse_a_null_handle():
    import blingfire_amd as bf
    hdr = open(os.path.join(bfutil.ROOT, "include", "blingfiretokdll_amd.h")).read()
    exports = open(os.path.join(bfutil.ROOT, "blingfire_amd", "csrc", "exports.map")).read()
    lib = ctypes.CDLL(bf.LIB_PATH)
    for name, nargs in (("IdsToMinHashBatchDevice", 15), ("IdsToMinHashBatch", 13), ("MinHashPairsBatchDevice", 8)):
        assert re.search(r"BF_API\s+\w+\s+%s\(" % name, hdr) and re.search(r"^\s*%s;" % name, exports, flags=re.M)
        assert name in bf._SIGNATURES and len(bf._SIGNATURES[name][1]) == nargs
        assert name in hdr[hdr.index("Status word of the last batch call"):hdr.index("BF_API int BfLastStatus")]
        assert getattr(lib, name)(*[None] * nargs) == -1      # refused without a device
    assert "bf_kernels_minhash.hip" in open(os.path.join(bfutil.ROOT, "blingfire_amd", "build.py")).read()
