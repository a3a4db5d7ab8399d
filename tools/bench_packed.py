"""MEASUREMENT: the packed stage (IdsToPackedRowsBatchDevice: ragged ids -> [R, L] ids + segment ids + position ids, several sequences per row)
beside the rows stage on the same ids at the same L and a plain copy.

1 M documents of bfutil.gen_corpus (workload config2) under bert_base_tok.bin, tokenised once (TextToIdsBatchDevice); the ids stay resident on
the device.  For L = 128 and L = 512, [CLS] / [SEP] set: every plane, row start, sequence row / cell and the row count of the packed stage is
verified first against the restatement of the specification (tests/packed_cases.py, the sequential greedy loop) applied to the same ids.  Then
three things are timed in this process, in alternating windows of at least one second each (device events around a window, calls back to back
on one stream with one synchronisation per 8 calls, a warm-up call of each before the first window), median of `--windows` windows with the
spread:

  packed     IdsToPackedRowsBatchDevice with every output and rows_cap = R (nothing is read back)
  rows       IdsToRowsBatchDevice, one row per document, all four outputs and the row offsets: the cost of the geometry is packed against this
  copy       one hipMemcpyAsync, device to device, of as many bytes as the packed stage writes: the fill is held against this

and, from the events the packed call records on its stream (BfLastKernelMs, median of 21 synchronised calls): widths + scan, next, the doubling
rounds together, the scan of the marks with the per-row / per-sequence outputs, the fill.  The real-cell share of both outputs is counted on the
device.  Writes profiles/packed_bench.json.

  python tools/bench_packed.py [--docs 1000000] [--windows 5] [--out profiles/packed_bench.json]"""
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
    ap.add_argument("--row-lens", type=int, nargs="+", default=[128, 512])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "packed_bench.json"))
    a = ap.parse_args()

    import torch
    import bfutil
    import blingfire_amd as bf
    import packed_cases as pc

    if not torch.cuda.is_available():
        sys.exit("bench_packed.py measures on the GPU: no device is visible")
    VP = ctypes.c_void_p
    CLS, SEP, PAD, UNK = 101, 102, 0, 100
    wl = bfutil.WORKLOADS["config2"]
    text, off = bfutil.gen_corpus(a.docs, **wl["gen"])
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

    # the ids, once: every document up to the ids the longest row can hold (a WordPiece model never yields more ids than bytes)
    max_len = max(a.row_lens) - 2
    ids_cap = min(total, n * max_len) + 1
    d_ids = torch.empty(ids_cap, dtype=torch.int32, device=dev)
    d_idoff = torch.empty(n + 1, dtype=torch.int64, device=dev)
    assert lib.TextToIdsBatchDevice(VP(h), d_text.data_ptr(), d_off.data_ptr(), n, total, d_ids.data_ptr(), ids_cap, d_idoff.data_ptr(), max_len, UNK, sp) == 0
    torch.cuda.synchronize()
    assert lib.BfLastStatus(VP(h)) == 0
    idoff_h = d_idoff.cpu().numpy()
    nids = int(idoff_h[-1])
    ids_h = d_ids.cpu().numpy()[:nids]
    del d_text

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

    res = {"docs": n, "text_bytes": total, "ids": nids, "model": "bert_base_tok.bin", "workload": "config2", "verified": True,
           "device": torch.cuda.get_device_name(0), "window_seconds": a.window_seconds, "row_lens": {}}
    for L in a.row_lens:
        d_nrows = torch.zeros(1, dtype=torch.int64, device=dev)
        pre = (VP(h), d_ids.data_ptr(), ids_cap, d_idoff.data_ptr(), n, L, CLS, SEP, PAD, 0)
        assert lib.IdsToPackedRowsBatchDevice(*pre, None, None, None, None, 0, None, None, d_nrows.data_ptr(), sp) == 0      # the size query
        R = int(d_nrows.item())
        planes = [torch.empty((R, L), dtype=torch.int32, device=dev) for _ in range(3)]
        d_first = torch.empty(R + 1, dtype=torch.int32, device=dev)
        d_seq = [torch.empty(n, dtype=torch.int32, device=dev) for _ in range(2)]
        packed_bytes = 3 * R * L * 4 + (R + 1) * 4 + 2 * n * 4 + 8
        r_rows = torch.empty((n, L), dtype=torch.int32, device=dev)
        r_mask = torch.empty((n, L), dtype=torch.uint8, device=dev)
        r_seq, r_first = torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
        r_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
        rows_bytes = n * L * 5 + 2 * n * 4 + (n + 1) * 8
        d_src = torch.zeros(packed_bytes, dtype=torch.uint8, device=dev)
        d_dst = torch.empty(packed_bytes, dtype=torch.uint8, device=dev)

        def packed():
            r = lib.IdsToPackedRowsBatchDevice(*pre, planes[0].data_ptr(), planes[1].data_ptr(), planes[2].data_ptr(), d_first.data_ptr(), R, d_seq[0].data_ptr(),
                                               d_seq[1].data_ptr(), d_nrows.data_ptr(), sp)
            assert r == 0, r

        def rows():
            r = lib.IdsToRowsBatchDevice(VP(h), d_ids.data_ptr(), ids_cap, d_idoff.data_ptr(), n, L, CLS, SEP, PAD, 0, 1, 0, r_rows.data_ptr(), r_mask.data_ptr(),
                                         r_seq.data_ptr(), r_first.data_ptr(), n, r_off.data_ptr(), sp)
            assert r == 0, r

        def copy():
            r = hip.hipMemcpyAsync(d_dst.data_ptr(), d_src.data_ptr(), packed_bytes, 3, sp)      # 3 = hipMemcpyDeviceToDevice
            assert r == 0, r

        # warm-up, and the run that is verified
        packed(); rows(); copy()
        torch.cuda.synchronize()
        assert lib.BfLastStatus(VP(h)) == 0
        want = pc.restate(ids_h, idoff_h, L, CLS, SEP, PAD)
        assert want[6] == R and int(d_nrows.item()) == R, "the row count differs from the restatement"
        for name, got, w in zip(("rows", "seg", "pos", "row_first_seq", "seq_row", "seq_col"), (*planes, d_first, *d_seq), want):
            assert np.array_equal(got.cpu().numpy(), w), "%s differ from the restatement" % name
        del want
        real_packed = int((planes[1] != 0).sum().item())
        real_rows = int(r_mask.sum(dtype=torch.int64).item())

        # the stages of one packed call, from the events it records
        stages = []
        buf = (ctypes.c_float * 6)()
        for _ in range(21):
            packed()
            assert lib.BfLastKernelMs(VP(h), buf, 6) == 6
            stages.append([buf[i] for i in range(6)])
        st = [statistics.median(s[i] for s in stages) for i in range(6)]

        times = {"packed": [], "rows": [], "copy": []}
        for _ in range(a.windows):
            for name, fn in (("packed", packed), ("rows", rows), ("copy", copy)):
                times[name].append(window(fn))
        med = {k: statistics.median(v) for k, v in times.items()}
        res["row_lens"][str(L)] = {
            "row_len": L, "packed_rows": R, "rows_stage_rows": n,
            "real_cell_share": {"packed": real_packed / (R * L), "rows_stage": real_rows / (n * L)},
            "packed": summary(times["packed"]), "rows": summary(times["rows"]), "copy": summary(times["copy"]),
            "packed_stages_ms": {"widths_scan": st[0], "next": st[1] - st[5], "doubling_rounds": st[5], "rounds": n.bit_length(),
                                 "marks_scan_rows_cols": st[2], "fill": st[3], "total": st[4]},
            "packed_bytes_written": packed_bytes, "rows_bytes_written": rows_bytes,
            "packed_written_GBps": packed_bytes / med["packed"] / 1e6, "rows_written_GBps": rows_bytes / med["rows"] / 1e6, "copy_GBps": packed_bytes / med["copy"] / 1e6,
            "packed_over_rows": med["packed"] / med["rows"], "packed_over_copy": med["packed"] / med["copy"],
            "fill_over_copy": st[3] / med["copy"], "chain_over_fill": (st[1] + st[2]) / st[3] if st[3] > 0 else None,
            "docs_per_s": {"packed": n / med["packed"] * 1e3, "rows": n / med["rows"] * 1e3}}
        del planes, r_rows, r_mask, d_src, d_dst
        torch.cuda.empty_cache()
    bf.free_model(h)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
