"""MEASUREMENT: the pair stage (IdsToPairRowsBatchDevice: two ragged id batches -> [rows, L] ids + mask + type ids) beside a plain copy of the
bytes it writes and the rows stage at the same L and row count.

1 M + 1 documents of bfutil.gen_corpus (workload config2) under bert_base_tok.bin are tokenised once on the device (max_len = L - 3, what the
encode_pairs chain asks for in mode 1); pair q is A = document q, B = document q + 1, both sides read from that one id array.  L = 128,
[CLS] / [SEP] set, one row per pair, in two forms:

  pairs_mode0   mode 0, max_a = 32, stride 0, max_rows_per_pair 1 (the question kept, the context truncated)
  pairs_mode1   mode 1 (longest first)

Every row, mask byte, type byte, pair index, first-B index and offset of both forms is verified first against the restatement of the
specification (tests/pair_cases.py).  Then four things are timed in this process, in alternating windows of at least one second each (device
events around a window, calls back to back on one stream with one synchronisation per 8 calls, a warm-up call of each before the first
window), median of `--windows` windows with the spread:

  pairs_mode0, pairs_mode1   all five outputs and the row offsets
  copy                       one hipMemcpyAsync, device to device, of as many bytes as the pair stage writes
  rows                       the unchanged IdsToRowsBatchDevice over the A side at the same L and row count, beside a copy of ITS bytes (rows_copy)

Writes profiles/pairs_bench.json.

  python tools/bench_pairs.py [--pairs 1000000] [--windows 5] [--out profiles/pairs_bench.json]"""
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
    ap.add_argument("--pairs", type=int, default=1000000)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--window-seconds", type=float, default=1.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pairs_bench.json"))
    a = ap.parse_args()

    import torch
    import bfutil
    import blingfire_amd as bf
    import pair_cases as pc

    if not torch.cuda.is_available():
        sys.exit("bench_pairs.py measures on the GPU: no device is visible")
    VP = ctypes.c_void_p
    L, CLS, SEP, PAD, UNK, MAX_A = 128, 101, 102, 0, 100, 32
    wl = bfutil.WORKLOADS["config2"]
    n = a.pairs
    text, off = bfutil.gen_corpus(n + 1, **wl["gen"])
    total = int(off[-1])
    lib = bf.lib()
    h = bf.load_model(bfutil.model_path("bert_base_tok.bin"))
    dev = torch.device("cuda:0")
    d_text, d_off = torch.from_numpy(text).to(dev), torch.from_numpy(off).to(dev)
    max_len = L - 3
    ids_cap = (n + 1) * max_len
    d_ids = torch.empty(ids_cap, dtype=torch.int32, device=dev)
    d_idoff = torch.empty(n + 2, dtype=torch.int64, device=dev)
    d_offa, d_offb = d_idoff[:n + 1], d_idoff[1:]
    d_rows = torch.empty((n, L), dtype=torch.int32, device=dev)
    d_mask = torch.empty((n, L), dtype=torch.uint8, device=dev)
    d_type = torch.empty((n, L), dtype=torch.uint8, device=dev)
    d_seq = torch.empty(n, dtype=torch.int32, device=dev)
    d_first = torch.empty(n, dtype=torch.int32, device=dev)
    d_roff = torch.empty(n + 1, dtype=torch.int64, device=dev)
    rows_bytes = d_rows.numel() * 4 + d_mask.numel() + d_seq.numel() * 4 + d_first.numel() * 4 + d_roff.numel() * 8
    pairs_bytes = rows_bytes + d_type.numel()
    d_src = torch.zeros(pairs_bytes, dtype=torch.uint8, device=dev)
    d_dst = torch.empty(pairs_bytes, dtype=torch.uint8, device=dev)
    assert lib.BfReserve(VP(h), n + 1, total, 0) == 0
    stream = torch.cuda.current_stream()
    sp = VP(stream.cuda_stream)
    hip = ctypes.CDLL("libamdhip64.so")                         # the HIP runtime torch and the library already run on
    hip.hipMemcpyAsync.restype = ctypes.c_int
    hip.hipMemcpyAsync.argtypes = [VP, VP, ctypes.c_size_t, ctypes.c_int, VP]

    r = lib.TextToIdsBatchDevice(VP(h), d_text.data_ptr(), d_off.data_ptr(), n + 1, total, d_ids.data_ptr(), ids_cap, d_idoff.data_ptr(), max_len, UNK, sp)
    assert r == 0, r
    torch.cuda.synchronize()
    assert lib.BfLastStatus(VP(h)) == 0

    def pairs(mode, max_a):
        r = lib.IdsToPairRowsBatchDevice(VP(h), d_ids.data_ptr(), ids_cap, d_offa.data_ptr(), d_ids.data_ptr(), ids_cap, d_offb.data_ptr(), n, L, CLS, SEP, PAD,
                                         mode, max_a, 0, 1, 0, d_rows.data_ptr(), d_mask.data_ptr(), d_type.data_ptr(), d_seq.data_ptr(), d_first.data_ptr(), n,
                                         d_roff.data_ptr(), sp)
        assert r == 0, r

    def pairs_mode0():
        pairs(0, MAX_A)

    def pairs_mode1():
        pairs(1, 0)

    def rows():
        r = lib.IdsToRowsBatchDevice(VP(h), d_ids.data_ptr(), ids_cap, d_offa.data_ptr(), n, L, CLS, SEP, PAD, 0, 1, 0, d_rows.data_ptr(), d_mask.data_ptr(),
                                     d_seq.data_ptr(), d_first.data_ptr(), n, d_roff.data_ptr(), sp)
        assert r == 0, r

    def copy():
        r = hip.hipMemcpyAsync(d_dst.data_ptr(), d_src.data_ptr(), pairs_bytes, 3, sp)      # 3 = hipMemcpyDeviceToDevice
        assert r == 0, r

    def rows_copy():
        r = hip.hipMemcpyAsync(d_dst.data_ptr(), d_src.data_ptr(), rows_bytes, 3, sp)
        assert r == 0, r

    # warm-up, and the runs that are verified
    ids_h, idoff_h = d_ids.cpu().numpy(), d_idoff.cpu().numpy()
    ids_h = ids_h[:int(idoff_h[-1])]
    kept = {}
    for name, fn, mode, max_a in (("pairs_mode0", pairs_mode0, 0, MAX_A), ("pairs_mode1", pairs_mode1, 1, 0)):
        fn()
        torch.cuda.synchronize()
        assert lib.BfLastStatus(VP(h)) == 0
        want = pc.restate_one_row(ids_h, idoff_h[:-1], ids_h, idoff_h[1:], L, CLS, SEP, PAD, mode, max_a)
        for what, got, w in zip(("rows", "mask", "type", "row_seq", "row_first_b", "row_offsets"), (d_rows, d_mask, d_type, d_seq, d_first, d_roff), want):
            assert np.array_equal(got.cpu().numpy(), w), "%s: %s differ from the restatement" % (name, what)
        kept[name] = {"ids_per_row": float(want[1].sum()) / n - 3, "type1_per_row": float(want[2].sum()) / n}
        del want
    rows(); copy(); rows_copy()
    torch.cuda.synchronize()

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

    fns = (("pairs_mode0", pairs_mode0), ("pairs_mode1", pairs_mode1), ("copy", copy), ("rows", rows), ("rows_copy", rows_copy))
    times = {name: [] for name, _ in fns}
    for _ in range(a.windows):
        for name, fn in fns:
            times[name].append(window(fn))
    bf.free_model(h)

    def summary(v):
        return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "windows": len(v)}
    med = {k: statistics.median(v) for k, v in times.items()}
    res = {"pairs": n, "text_bytes": total, "ids": int(idoff_h[-1]), "model": "bert_base_tok.bin", "workload": "config2", "row_len": L, "max_len": max_len,
           "mode0_max_a": MAX_A, "verified": True, "device": torch.cuda.get_device_name(0), "window_seconds": a.window_seconds, "kept": kept}
    for name in times:
        res[name] = summary(times[name])
    res.update({"pairs_bytes_written": pairs_bytes, "rows_bytes_written": rows_bytes,
                "pairs_mode0_written_GBps": pairs_bytes / med["pairs_mode0"] / 1e6, "pairs_mode1_written_GBps": pairs_bytes / med["pairs_mode1"] / 1e6,
                "copy_GBps": pairs_bytes / med["copy"] / 1e6,
                "pairs_mode0_over_copy": med["pairs_mode0"] / med["copy"], "pairs_mode1_over_copy": med["pairs_mode1"] / med["copy"],
                "rows_over_rows_copy": med["rows"] / med["rows_copy"],
                "pairs_mode0_over_rows": med["pairs_mode0"] / med["rows"], "pairs_mode1_over_rows": med["pairs_mode1"] / med["rows"],
                "pairs_per_s": {"pairs_mode0": n / med["pairs_mode0"] * 1e3, "pairs_mode1": n / med["pairs_mode1"] * 1e3}})
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
