"""MEASUREMENT: the decontamination path -- IdsToNgramSetBatchDevice and IdsNgramOverlapBatchDevice beside IdsToMinHashBatchDevice and
TextToIdsBatchDevice on the same batch, a plain copy, and the torch formulation.

`--docs` documents of bfutil.gen_corpus (workload config2) under bert_base_tok.bin, tokenised once on the device (max_len 128); n = 13.  The set
is built from the first hundredth of the same documents, so one document in a hundred is contaminated through and through and the rest hit by
chance only.  Verified before anything is timed: a set of the first `--verify-set-docs` documents and every output of the overlap call over the
first `--verify-docs` against tests/ngram_cases (counts, ngrams, hits, covered, mask), and on the full batch that every n-gram of the set's own
documents hits.  Then, in this process, in alternating windows of at least one second each (device events around a window, calls back to back
on one stream with one synchronisation per 8 calls, a warm-up call of each before the first window), median of `--windows` windows with the spread:

  set           IdsToNgramSetBatchDevice over the hundredth, table cleared by the call (2 * ids + 64 slots of the slice)
  overlap       IdsNgramOverlapBatchDevice over the batch: ngrams, hits, covered
  overlap_mask  the same with the per-id mask taken too
  signatures    IdsToMinHashBatchDevice on the same ids (num_perm 128, shingle 5, band_rows 8)
  tokenize      TextToIdsBatchDevice on the batch
  copy          one hipMemcpyAsync, device to device, of the bytes every overlap call reads whatever the data: the ids and the offsets (the
                table is gathered from, not streamed, and is not counted)
  torch         unfold over the first `--torch-ids` ids, the same fingerprint in int64 tensor ops, torch.isin against the set's fingerprints.
                It ignores where sequences end and yields the hit flag per start only: no counts per sequence, no coverage

Not measured here: hardware counters, the LDS bank behaviour of the skewed staging block, n = 64.  Writes profiles/ngram_bench.json.

  python tools/bench_ngram.py [--docs 1000000] [--windows 5] [--out profiles/ngram_bench.json]"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1000000)
    ap.add_argument("--verify-docs", type=int, default=2000)
    ap.add_argument("--verify-set-docs", type=int, default=300)
    ap.add_argument("--torch-ids", type=int, default=50000000)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--window-seconds", type=float, default=1.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ngram_bench.json"))
    a = ap.parse_args()

    import torch
    import bfutil
    import blingfire_amd as bf
    import ngram_cases as nc

    if not torch.cuda.is_available():
        sys.exit("bench_ngram.py measures on the GPU: no device is visible")
    VP = ctypes.c_void_p
    N, SEED, L, UNK = 13, 0, 128, 100
    text, off = bfutil.gen_corpus(a.docs, **bfutil.WORKLOADS["config2"]["gen"])
    n, total = a.docs, int(off[-1])
    nset = max(1, n // 100)
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

    def tokenize():
        r = lib.TextToIdsBatchDevice(VP(h), d_text.data_ptr(), d_off.data_ptr(), n, total, d_ids.data_ptr(), ids_cap, d_idoff.data_ptr(), L, UNK, sp)
        assert r == 0, r

    def status():
        torch.cuda.synchronize()
        return lib.BfLastStatus(VP(h))

    tokenize()
    assert status() == 0
    idoff_h = d_idoff.cpu().numpy()
    nids, set_ids = int(idoff_h[-1]), int(idoff_h[nset])
    table = torch.empty(2 * set_ids + 64, dtype=torch.int64, device=dev)
    counts = torch.empty(3, dtype=torch.int64, device=dev)
    ngrams, hits, covered = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(3))
    mask = torch.empty(ids_cap, dtype=torch.uint8, device=dev)
    H, K, R = 128, 5, 8
    sig, keys, nsh = torch.empty((n, H), dtype=torch.int32, device=dev), torch.empty((n, H // R), dtype=torch.int64, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
    copy_bytes = nids * 4 + (n + 1) * 8
    d_src, d_dst = torch.zeros(copy_bytes, dtype=torch.uint8, device=dev), torch.empty(copy_bytes, dtype=torch.uint8, device=dev)

    def set_call(docs=nset):
        r = lib.IdsToNgramSetBatchDevice(VP(h), d_ids.data_ptr(), ids_cap, d_idoff.data_ptr(), docs, N, SEED, 1, table.data_ptr(), table.numel(), counts.data_ptr(), sp)
        assert r == 0, r

    def overlap(docs=n, m=None):
        r = lib.IdsNgramOverlapBatchDevice(VP(h), d_ids.data_ptr(), ids_cap, d_idoff.data_ptr(), docs, N, SEED, 0, table.data_ptr(), table.numel(), ngrams.data_ptr(),
                                           hits.data_ptr(), covered.data_ptr(), None if m is None else m.data_ptr(), sp)
        assert r == 0, r

    def overlap_mask():
        overlap(n, mask)

    def signatures():
        r = lib.IdsToMinHashBatchDevice(VP(h), d_ids.data_ptr(), ids_cap, d_idoff.data_ptr(), n, K, H, R, 0, 0, sig.data_ptr(), n, keys.data_ptr(), nsh.data_ptr(), sp)
        assert r == 0, r

    def copy():
        r = hip.hipMemcpyAsync(d_dst.data_ptr(), d_src.data_ptr(), copy_bytes, 3, sp)      # 3 = hipMemcpyDeviceToDevice
        assert r == 0, r

    def s64(x):                                                 # a uint64 constant as the int64 of the same bits
        x &= 0xFFFFFFFFFFFFFFFF
        return x - (1 << 64) if x >> 63 else x

    def fmix(x):                                                # fmix64 on int64 tensors: the shifts made logical by a mask
        x = (x ^ ((x >> 33) & 0x7FFFFFFF)) * s64(0xFF51AFD7ED558CCD)
        x = (x ^ ((x >> 33) & 0x7FFFFFFF)) * s64(0xC4CEB9FE1A85EC53)
        return x ^ ((x >> 33) & 0x7FFFFFFF)

    def torch_prints(ids):
        m = fmix(((ids.long() & 0xFFFFFFFF) + 1) * s64(0x9E3779B97F4A7C15) ^ s64(SEED)).unfold(0, N, 1)
        P = torch.zeros(m.shape[0], dtype=torch.int64, device=ids.device)
        for i in range(N):
            P = P * 0x100000001B3 + m[:, i]
        return fmix(P ^ s64(N * 0xC2B2AE3D27D4EB4F))

    nt = min(nids, a.torch_ids)
    set_prints = torch.unique(torch_prints(d_ids[:set_ids]))

    def torch_form():
        torch.isin(torch_prints(d_ids[:nt]), set_prints)

    # verified first: a small set and a slice of the batch against the restatement, then the set's own documents on the full table
    ns, nv = min(nset, a.verify_set_docs), min(n, a.verify_docs)
    ids_h = d_ids[:int(idoff_h[nv])].cpu().numpy()
    members, want_counts = nc.build(ids_h, idoff_h[:ns + 1], N, SEED)
    set_call(ns)
    overlap(nv, mask)
    assert status() == 0 and counts.cpu().tolist() == want_counts.tolist()
    want = nc.overlap(ids_h, idoff_h[:nv + 1], N, SEED, members)
    for name, g in zip(("ngrams", "hits", "covered"), (ngrams, hits, covered)):
        assert np.array_equal(g[:nv].cpu().numpy(), want[name]), "%s differ from the restatement" % name
    assert np.array_equal(mask[:len(ids_h)].cpu().numpy(), want["mask"]), "mask differs from the restatement"
    first = torch_prints(d_ids[:int(idoff_h[1])])               # the torch fingerprint is the library's: the first document's are all in the set
    assert idoff_h[1] < N or bool(torch.isin(first, torch.from_numpy(np.array(sorted(members), dtype=np.uint64).view(np.int64)).to(dev)).all())
    set_call()
    overlap()
    assert status() == 0
    full_counts = [int(x) for x in counts.tolist()]
    assert full_counts[2] == 0 and torch.equal(hits[:nset], ngrams[:nset])
    found = {"contaminated_docs": int((hits > 0).sum()), "hit_ngrams": int(hits.sum()), "ngrams": int(ngrams.sum()), "covered_ids": int(covered.sum())}

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

    fns = (("set", set_call), ("overlap", overlap), ("overlap_mask", overlap_mask), ("signatures", signatures), ("tokenize", tokenize), ("copy", copy), ("torch", torch_form))
    for _, fn in fns:
        fn()
    assert status() == 0
    times = {name: [] for name, _ in fns}
    for _ in range(a.windows):
        for name, fn in fns:
            times[name].append(window(fn))
    med = {k: statistics.median(v) for k, v in times.items()}
    res = {"docs": n, "text_bytes": total, "ids": nids, "model": "bert_base_tok.bin", "workload": "config2", "ngram": N, "max_len": L, "set_docs": nset, "set_ids": set_ids,
           "table_slots": table.numel(), "device": torch.cuda.get_device_name(0), "window_seconds": a.window_seconds,
           "verified": "the set call's counts over the first %d documents and every output of the overlap call over the first %d against tests/ngram_cases; "
                       "on the full batch, hits == ngrams for the set's own documents" % (ns, nv),
           "set_counts": {"read": full_counts[0], "stored": full_counts[1], "no_slot": full_counts[2]}, "overlap_found": found,
           **{name: summary(v) for name, v in times.items()},
           "copy_bytes": copy_bytes, "overlap_over_copy": med["overlap"] / med["copy"], "overlap_over_signatures": med["overlap"] / med["signatures"],
           "overlap_over_tokenize": med["overlap"] / med["tokenize"], "torch_ids": nt, "torch_ms_per_million_ids": med["torch"] / nt * 1e6,
           "overlap_ms_per_million_ids": med["overlap"] / nids * 1e6,
           "torch_note": "unfold + int64 fingerprint + torch.isin over torch_ids ids: the hit flag per start only, sequence ends ignored",
           "ids_per_s": {name: (set_ids if name == "set" else nids) / med[name] * 1e3 for name in ("set", "overlap", "overlap_mask", "signatures")},
           "not_measured": "hardware counters, the LDS bank behaviour of the skewed staging block, n = 64"}
    bf.free_model(h)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
