"""MEASUREMENT: the near-duplicate path -- IdsToMinHashBatchDevice (signatures, band keys) beside TextToIdsBatchDevice on the same batch, and
MinHashClustersBatchDevice beside a torch baseline and a plain copy.

`--docs` documents of bfutil.gen_corpus (workload config2) under bert_base_tok.bin, the last tenth of them replaced by planted near-duplicates
(copies of earlier documents, every second one with a word put in front); the text stays resident on the device.  num_perm = 128, shingle = 5,
band_rows = 8 (16 bands), max_len = 128, min_equal = 103 (a Jaccard estimate of 0.8).  Verified before anything is timed: signatures, keys and
shingle counts of the first `--verify-sig-docs` documents against tests/minhash_cases.restate, and label, keep, size and counts of the clusters
call over the first `--verify-docs` documents (on the device's own keys and signatures) against tests/mhclust_cases.restate, with and without
min_equal (the planted copies sit in the last tenth, so with the default sizes that slice holds no candidate: `verified_counts` in the result says
what it held; candidates are the GPU tests' to verify).  Then, in this process, in alternating windows of at least one second each (device events around a window, calls back to back on one
stream with one synchronisation per 8 calls, a warm-up call of each before the first window), median of `--windows` windows with the spread:

  tokenize    TextToIdsBatchDevice on the batch
  signatures  IdsToMinHashBatchDevice on its ids: signatures, band keys, shingle counts
  clusters    MinHashClustersBatchDevice on those, min_equal = 103, every output taken
  clusters_0  the same with min_equal = 0 (no signature is read)
  torch_sort  torch.sort of the same nseq x 16 keys and unique_consecutive over them.  This baseline yields only the band GROUPS: neither the
              verified links nor the components, which the clusters call ends with
  copy        one hipMemcpyAsync, device to device, of the bytes every clusters call reads whatever the data: the keys and the shingle counts

and the stages of one clusters call from the events it records (BfLastKernelMs, median of 21 synchronised calls).  Writes profiles/minhash_bench.json.

  python tools/bench_minhash.py [--docs 1000000] [--windows 5] [--out profiles/minhash_bench.json]"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def plant(text, off, rng):
    """the last tenth of the documents become copies of earlier ones, every second one with a word in front"""
    n = len(off) - 1
    first = n - n // 10
    docs = [text[off[i]:off[i + 1]] for i in range(first)]
    word = np.frombuffer(b"zebra ", dtype=np.uint8)
    for j, src in enumerate(rng.integers(0, first, size=n - first).tolist()):
        docs.append(np.concatenate([word, docs[src]]) if j & 1 else docs[src])
    out_off = np.zeros(n + 1, dtype=np.int64)
    np.cumsum([len(d) for d in docs], out=out_off[1:])
    return np.concatenate(docs), out_off


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1000000)
    ap.add_argument("--verify-docs", type=int, default=100000)
    ap.add_argument("--verify-sig-docs", type=int, default=2000)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--window-seconds", type=float, default=1.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "minhash_bench.json"))
    a = ap.parse_args()

    import torch
    import bfutil
    import blingfire_amd as bf
    import mhclust_cases as cc
    import minhash_cases as mc

    if not torch.cuda.is_available():
        sys.exit("bench_minhash.py measures on the GPU: no device is visible")
    VP = ctypes.c_void_p
    H, K, R, L, UNK, ME = 128, 5, 8, 128, 100, 103
    B = H // R
    text, off = plant(*bfutil.gen_corpus(a.docs, **bfutil.WORKLOADS["config2"]["gen"]), np.random.default_rng(1))
    n, total = a.docs, int(off[-1])
    lib = bf.lib()
    h = bf.load_model(bfutil.model_path("bert_base_tok.bin"))
    dev = torch.device("cuda:0")
    d_text, d_off = torch.from_numpy(text).to(dev), torch.from_numpy(off).to(dev)
    assert lib.BfReserve(VP(h), n, total, 0) == 0
    stream = torch.cuda.current_stream()
    sp = VP(stream.cuda_stream)
    hip = ctypes.CDLL("libamdhip64.so")                         # the HIP runtime torch and the library already run on
    hip.hipMemcpyAsync.restype = ctypes.c_int
    hip.hipMemcpyAsync.argtypes = [VP, VP, ctypes.c_size_t, ctypes.c_int, VP]

    ids_cap = min(total, n * L) + 1
    d_ids = torch.empty(ids_cap, dtype=torch.int32, device=dev)
    d_idoff = torch.empty(n + 1, dtype=torch.int64, device=dev)
    sig = torch.empty((n, H), dtype=torch.int32, device=dev)
    keys = torch.empty((n, B), dtype=torch.int64, device=dev)
    nsh, label, size = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(3))
    keep, counts = torch.empty(n, dtype=torch.uint8, device=dev), torch.empty(2, dtype=torch.int64, device=dev)
    copy_bytes = n * B * 8 + n * 4
    d_src, d_dst = torch.zeros(copy_bytes, dtype=torch.uint8, device=dev), torch.empty(copy_bytes, dtype=torch.uint8, device=dev)

    def tokenize():
        r = lib.TextToIdsBatchDevice(VP(h), d_text.data_ptr(), d_off.data_ptr(), n, total, d_ids.data_ptr(), ids_cap, d_idoff.data_ptr(), L, UNK, sp)
        assert r == 0, r

    def signatures():
        r = lib.IdsToMinHashBatchDevice(VP(h), d_ids.data_ptr(), ids_cap, d_idoff.data_ptr(), n, K, H, R, 0, 0, sig.data_ptr(), n, keys.data_ptr(), nsh.data_ptr(), sp)
        assert r == 0, r

    def clusters(me=ME, rows=None):
        m = n if rows is None else rows
        r = lib.MinHashClustersBatchDevice(VP(h), sig.data_ptr(), H, keys.data_ptr(), B, m, nsh.data_ptr(), me, 0, label.data_ptr(), keep.data_ptr(), size.data_ptr(),
                                           counts.data_ptr(), sp)
        assert r == 0, r

    def clusters_0():
        clusters(0)

    def torch_sort():
        torch.unique_consecutive(torch.sort(keys.flatten())[0])

    def copy():
        r = hip.hipMemcpyAsync(d_dst.data_ptr(), d_src.data_ptr(), copy_bytes, 3, sp)      # 3 = hipMemcpyDeviceToDevice
        assert r == 0, r

    def status():
        torch.cuda.synchronize()
        return lib.BfLastStatus(VP(h))

    tokenize()
    assert status() == 0
    signatures()
    assert status() == 0
    idoff_h = d_idoff.cpu().numpy()
    ns = min(n, a.verify_sig_docs)
    want = mc.restate(d_ids[:int(idoff_h[ns])].cpu().numpy(), idoff_h[:ns + 1], K, H, R, 0)
    for name, g in zip(("sig", "keys", "nshingles"), (sig, keys, nsh)):
        assert np.array_equal(g[:ns].cpu().numpy(), want[name]), "%s differ from the restatement" % name
    nv = min(n, a.verify_docs)
    keys_h, sig_h, nsh_h = (x[:nv].cpu().numpy() for x in (keys, sig, nsh))
    found = {}
    for me in (0, ME):
        clusters(me, nv)
        assert status() == 0
        want = cc.restate(keys_h, sig_h, me, nsh_h)
        for name, g in zip(("label", "keep", "size", "counts"), (label[:nv], keep[:nv], size[:nv], counts)):
            assert np.array_equal(g.cpu().numpy(), want[name]), "%s differ from the restatement (min_equal %d)" % (name, me)
        found[me] = {"docs": nv, "clusters": int(want["counts"][0]), "candidates": int(want["counts"][1]), "rejected": want["rejected"]}

    def window(fn):
        reps = 0
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        while True:
            for _ in range(8):
                fn()
            reps += 8
            e1.record(stream)
            e1.synchronize()
            ms = e0.elapsed_time(e1)
            if ms >= a.window_seconds * 1e3:
                return ms / reps

    def summary(v):
        return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "windows": len(v)}

    fns = (("tokenize", tokenize), ("signatures", signatures), ("clusters", clusters), ("clusters_0", clusters_0), ("torch_sort", torch_sort), ("copy", copy))
    for _, fn in fns:
        fn()
    assert status() == 0
    clusters()
    torch.cuda.synchronize()
    full = [int(x) for x in counts.tolist()]
    stages, buf = [], (ctypes.c_float * 6)()
    for _ in range(21):
        clusters()
        assert lib.BfLastKernelMs(VP(h), buf, 6) == 6
        stages.append([buf[i] for i in range(6)])
    st = [statistics.median(s[i] for s in stages) for i in range(6)]
    times = {name: [] for name, _ in fns}
    for _ in range(a.windows):
        for name, fn in fns:
            times[name].append(window(fn))
    med = {k: statistics.median(v) for k, v in times.items()}
    res = {"docs": n, "text_bytes": total, "ids": int(idoff_h[-1]), "model": "bert_base_tok.bin", "workload": "config2 with a tenth of planted near-duplicates",
           "num_perm": H, "shingle": K, "band_rows": R, "bands": B, "max_len": L, "min_equal": ME, "device": torch.cuda.get_device_name(0),
           "window_seconds": a.window_seconds,
           "verified": "signatures, keys and shingle counts of the first %d documents, and every output of the clusters call over the first %d, against the restatements" % (ns, nv),
           "verified_counts": {str(k): v for k, v in found.items()}, "full_call_counts": {"clusters": full[0], "candidates": full[1]},
           **{name: summary(v) for name, v in times.items()},
           "clusters_stages_ms": {"begin": st[0], "bands": st[1], "flatten_sizes": st[3], "total": st[4]},
           "copy_bytes": copy_bytes, "clusters_over_copy": med["clusters"] / med["copy"], "clusters_over_torch_sort": med["clusters"] / med["torch_sort"],
           "torch_sort_note": "torch.sort + unique_consecutive yields the band groups only, not the verified links or the components",
           "signatures_over_tokenize": med["signatures"] / med["tokenize"],
           "docs_per_s": {name: n / med[name] * 1e3 for name in ("tokenize", "signatures", "clusters")}}
    bf.free_model(h)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
