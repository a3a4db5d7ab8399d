"""MEASUREMENT: the rows stage (IdsToRowsBatchDevice: ragged ids -> [rows, L] ids + mask) beside the tokenize step it follows and a plain copy.

1 M documents of bfutil.gen_corpus (workload config2) under bert_base_tok.bin, text and offsets resident on the device.  L = 64, [CLS] / [SEP]
set, one row per document: the tokenize step is TextToIdsBatchDevice at the max_len the chain uses (L - 2).  Every row, mask byte, row index and
offset of the rows stage is verified first against the restatement of the specification (tests/rows_cases.py) applied to the ids the tokenize
step produced.  Then three things are timed in this process, in alternating windows of at least one second each (device events around a window,
calls back to back on one stream with one synchronisation per 8 calls, a warm-up call of each before the first window), median of `--windows` windows with the spread:

  tokenize   TextToIdsBatchDevice alone
  rows       IdsToRowsBatchDevice alone (all four outputs and the row offsets)
  copy       one hipMemcpyAsync, device to device, of as many bytes as the rows stage writes

Writes profiles/rows_bench.json.

  python tools/bench_rows.py [--docs 1000000] [--windows 5] [--out profiles/rows_bench.json]"""
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
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--window-seconds", type=float, default=1.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rows_bench.json"))
    a = ap.parse_args()

    import torch
    import bfutil
    import blingfire_amd as bf
    import rows_cases as rc

    if not torch.cuda.is_available():
        sys.exit("bench_rows.py measures on the GPU: no device is visible")
    VP = ctypes.c_void_p
    L, CLS, SEP, PAD, UNK = 64, 101, 102, 0, 100
    wl = bfutil.WORKLOADS["config2"]
    text, off = bfutil.gen_corpus(a.docs, **wl["gen"])
    n, total = a.docs, int(off[-1])
    lib = bf.lib()
    h = bf.load_model(bfutil.model_path("bert_base_tok.bin"))
    dev = torch.device("cuda:0")
    d_text, d_off = torch.from_numpy(text).to(dev), torch.from_numpy(off).to(dev)
    max_len = L - 2
    ids_cap = n * max_len
    d_ids = torch.empty(ids_cap, dtype=torch.int32, device=dev)
    d_idoff = torch.empty(n + 1, dtype=torch.int64, device=dev)
    d_rows = torch.empty((n, L), dtype=torch.int32, device=dev)
    d_mask = torch.empty((n, L), dtype=torch.uint8, device=dev)
    d_seq = torch.empty(n, dtype=torch.int32, device=dev)
    d_first = torch.empty(n, dtype=torch.int32, device=dev)
    d_roff = torch.empty(n + 1, dtype=torch.int64, device=dev)
    rows_bytes = d_rows.numel() * 4 + d_mask.numel() + d_seq.numel() * 4 + d_first.numel() * 4 + d_roff.numel() * 8
    d_src = torch.zeros(rows_bytes, dtype=torch.uint8, device=dev)
    d_dst = torch.empty(rows_bytes, dtype=torch.uint8, device=dev)
    assert lib.BfReserve(VP(h), n, total, 0) == 0
    stream = torch.cuda.current_stream()
    sp = VP(stream.cuda_stream)
    hip = ctypes.CDLL("libamdhip64.so")                         # the HIP runtime torch and the library already run on
    hip.hipMemcpyAsync.restype = ctypes.c_int
    hip.hipMemcpyAsync.argtypes = [VP, VP, ctypes.c_size_t, ctypes.c_int, VP]

    def tokenize():
        r = lib.TextToIdsBatchDevice(VP(h), d_text.data_ptr(), d_off.data_ptr(), n, total, d_ids.data_ptr(), ids_cap, d_idoff.data_ptr(), max_len, UNK, sp)
        assert r == 0, r

    def rows():
        r = lib.IdsToRowsBatchDevice(VP(h), d_ids.data_ptr(), ids_cap, d_idoff.data_ptr(), n, L, CLS, SEP, PAD, 0, 1, 0, d_rows.data_ptr(), d_mask.data_ptr(),
                                     d_seq.data_ptr(), d_first.data_ptr(), n, d_roff.data_ptr(), sp)
        assert r == 0, r

    def copy():
        r = hip.hipMemcpyAsync(d_dst.data_ptr(), d_src.data_ptr(), rows_bytes, 3, sp)      # 3 = hipMemcpyDeviceToDevice
        assert r == 0, r

    # warm-up, and the run that is verified
    tokenize(); rows(); copy()
    torch.cuda.synchronize()
    assert lib.BfLastStatus(VP(h)) == 0
    ids_h, idoff_h = d_ids.cpu().numpy(), d_idoff.cpu().numpy()
    want = rc.restate_truncated(ids_h[:int(idoff_h[-1])], idoff_h, L, CLS, SEP, PAD)
    for name, got, w in zip(("rows", "mask", "row_seq", "row_first", "row_offsets"), (d_rows, d_mask, d_seq, d_first, d_roff), want):
        assert np.array_equal(got.cpu().numpy(), w), "%s differ from the restatement" % name
    del want, ids_h

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

    times = {"tokenize": [], "rows": [], "copy": []}
    for _ in range(a.windows):
        for name, fn in (("tokenize", tokenize), ("rows", rows), ("copy", copy)):
            times[name].append(window(fn))
    bf.free_model(h)

    def summary(v):
        return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "windows": len(v)}
    med = {k: statistics.median(v) for k, v in times.items()}
    res = {"docs": n, "text_bytes": total, "ids": int(idoff_h[-1]), "model": "bert_base_tok.bin", "workload": "config2", "row_len": L, "max_len": max_len,
           "verified": True, "device": torch.cuda.get_device_name(0), "window_seconds": a.window_seconds,
           "tokenize": summary(times["tokenize"]), "rows": summary(times["rows"]), "copy": summary(times["copy"]),
           "rows_bytes_written": rows_bytes, "rows_bytes_read": int(idoff_h[-1]) * 4 + (n + 1) * 8,
           "rows_written_GBps": rows_bytes / med["rows"] / 1e6, "copy_GBps": rows_bytes / med["copy"] / 1e6,
           "rows_over_tokenize": med["rows"] / med["tokenize"], "rows_over_copy": med["rows"] / med["copy"],
           "docs_per_s": {"tokenize": n / med["tokenize"] * 1e3, "rows": n / med["rows"] * 1e3, "tokenize_then_rows": n / (med["tokenize"] + med["rows"]) * 1e3}}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
