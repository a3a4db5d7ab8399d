"""MEASUREMENT: the bucketed stage (IdsToBucketedRowsBatchDevice: ragged ids -> length-sorted, budget-cut batches, each padded to its own longest
row) beside the rows stage on the same ids at L = max_len, a plain copy, and torch.sort on the same keys.

1 M documents of bfutil.gen_corpus (workload config2) under bert_base_tok.bin, tokenised once (TextToIdsBatchDevice); the ids stay resident on
the device.  For max_len = 128 and 512, [CLS] / [SEP] set, multiple = 8, max_cells = 16384.  Verified before anything is timed: every output of
the call over the first `--verify-docs` documents against the restatement of the specification (tests/bucketed_cases.py), and of the full call
`order` against torch.sort(stable) of the same keys, the batch chain against a host walk of the sorted widths, and the mask total against the
width total.  Then, in this process, in alternating windows of at least one second each (device events around a window, calls back to back on
one stream with one synchronisation per 8 calls, a warm-up call of each before the first window), median of `--windows` windows with the spread:

  bucketed   IdsToBucketedRowsBatchDevice with every output at exact caps (nothing is read back)
  rows       IdsToRowsBatchDevice, one row per document at L = max_len, all four outputs and the row offsets
  copy       one hipMemcpyAsync, device to device, of as many bytes as the two bucketed planes take
  torch_sort torch.sort(keys, stable=True) on the int32 keys max_len - width: the sort alone is held against slot [1] of BfLastKernelMs

and the stages of one call from the events it records (BfLastKernelMs, median of 21 synchronised calls).  Writes profiles/bucketed_bench.json.

  python tools/bench_bucketed.py [--docs 1000000] [--windows 5] [--out profiles/bucketed_bench.json]"""
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
    ap.add_argument("--verify-docs", type=int, default=100000)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--window-seconds", type=float, default=1.0)
    ap.add_argument("--max-lens", type=int, nargs="+", default=[128, 512])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bucketed_bench.json"))
    a = ap.parse_args()

    import torch
    import bfutil
    import blingfire_amd as bf
    import bucketed_cases as bc

    if not torch.cuda.is_available():
        sys.exit("bench_bucketed.py measures on the GPU: no device is visible")
    VP = ctypes.c_void_p
    CLS, SEP, PAD, UNK, MULT, CELLS = 101, 102, 0, 100, 8, 16384
    text, off = bfutil.gen_corpus(a.docs, **bfutil.WORKLOADS["config2"]["gen"])
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

    body = max(a.max_lens) - 2
    ids_cap = min(total, n * body) + 1
    d_ids = torch.empty(ids_cap, dtype=torch.int32, device=dev)
    d_idoff = torch.empty(n + 1, dtype=torch.int64, device=dev)
    assert lib.TextToIdsBatchDevice(VP(h), d_text.data_ptr(), d_off.data_ptr(), n, total, d_ids.data_ptr(), ids_cap, d_idoff.data_ptr(), body, UNK, sp) == 0
    torch.cuda.synchronize()
    assert lib.BfLastStatus(VP(h)) == 0
    idoff_h = d_idoff.cpu().numpy()
    nv = min(n, a.verify_docs)
    ids_v = d_ids[:int(idoff_h[nv])].cpu().numpy()
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

    res = {"docs": n, "text_bytes": total, "ids": int(idoff_h[-1]), "model": "bert_base_tok.bin", "workload": "config2", "multiple": MULT, "max_cells": CELLS,
           "verified": "every output over the first %d documents against the restatement; order, batch chain and mask total of the full call" % nv,
           "device": torch.cuda.get_device_name(0), "window_seconds": a.window_seconds, "max_lens": {}}
    for L in a.max_lens:
        # the call over the first documents, against the restatement
        got = bf.ids_to_bucketed_rows_batch_device(h, d_ids[:len(ids_v)], d_idoff[:nv + 1], L, CELLS, CLS, SEP, PAD, MULT)
        want = bc.restate(ids_v, idoff_h[:nv + 1], L, CLS, SEP, PAD, MULT, CELLS)
        for name, g in zip(("rows", "mask", "order", "seq_pos", "first", "len", "cell", "counts"), got):
            assert np.array_equal(g.cpu().numpy(), want[name]), "%s differ from the restatement" % name
        del got, want
        # the full call
        outs = list(bf.ids_to_bucketed_rows_batch_device(h, d_ids, d_idoff, L, CELLS, CLS, SEP, PAD, MULT))
        B, C = (int(x) for x in outs[7].tolist())
        pre = (VP(h), d_ids.data_ptr(), ids_cap, d_idoff.data_ptr(), n, L, CLS, SEP, PAD, MULT, CELLS, 0, 0)

        def bucketed():
            r = lib.IdsToBucketedRowsBatchDevice(*pre, outs[0].data_ptr(), outs[1].data_ptr(), C, *[o.data_ptr() for o in outs[2:7]], B, outs[7].data_ptr(), sp)
            assert r == 0, r
        width = torch.clamp(d_idoff[1:] - d_idoff[:-1], max=L - 2).to(torch.int32) + 2
        keys = (L - width).contiguous()
        assert torch.equal(torch.sort(keys, stable=True)[1].to(torch.int32), outs[2]), "order differs from torch.sort(stable)"
        ws, i, chain = width[outs[2].long()].cpu().numpy(), 0, []
        while i < n:
            chain.append(i)
            i += max(1, CELLS // max(MULT, bc.up(int(ws[i]), MULT)))
        assert chain + [n] == outs[4].tolist() and int(outs[1].sum(dtype=torch.int64).item()) == int(width.sum(dtype=torch.int64).item())
        r_rows = torch.empty((n, L), dtype=torch.int32, device=dev)
        r_mask = torch.empty((n, L), dtype=torch.uint8, device=dev)
        r_seq, r_first = torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
        r_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
        d_src, d_dst = torch.zeros(5 * C, dtype=torch.uint8, device=dev), torch.empty(5 * C, dtype=torch.uint8, device=dev)

        def rows():
            r = lib.IdsToRowsBatchDevice(VP(h), d_ids.data_ptr(), ids_cap, d_idoff.data_ptr(), n, L, CLS, SEP, PAD, 0, 1, 0, r_rows.data_ptr(), r_mask.data_ptr(),
                                         r_seq.data_ptr(), r_first.data_ptr(), n, r_off.data_ptr(), sp)
            assert r == 0, r

        def copy():
            r = hip.hipMemcpyAsync(d_dst.data_ptr(), d_src.data_ptr(), 5 * C, 3, sp)      # 3 = hipMemcpyDeviceToDevice
            assert r == 0, r

        def torch_sort():
            torch.sort(keys, stable=True)

        fns = (("bucketed", bucketed), ("rows", rows), ("copy", copy), ("torch_sort", torch_sort))
        for _, fn in fns:
            fn()
        torch.cuda.synchronize()
        assert lib.BfLastStatus(VP(h)) == 0
        real = int(width.sum(dtype=torch.int64).item())
        stages, buf = [], (ctypes.c_float * 6)()
        for _ in range(21):
            bucketed()
            assert lib.BfLastKernelMs(VP(h), buf, 6) == 6
            stages.append([buf[i] for i in range(6)])
        st = [statistics.median(s[i] for s in stages) for i in range(6)]
        times = {name: [] for name, _ in fns}
        for _ in range(a.windows):
            for name, fn in fns:
                times[name].append(window(fn))
        med = {k: statistics.median(v) for k, v in times.items()}
        res["max_lens"][str(L)] = {
            "max_len": L, "batches": B, "cells": C, "real_cell_share": {"bucketed": real / C, "rows_stage": real / (n * L)},
            **{name: summary(v) for name, v in times.items()},
            "stages_ms": {"keys": st[0], "sort_passes": st[1], "last_scatter": st[5], "chain_scans_batches": st[2], "fill": st[3], "total": st[4]},
            "plane_bytes": 5 * C, "fill_over_copy": st[3] / med["copy"], "sort_over_torch_sort": st[1] / med["torch_sort"],
            "bucketed_over_rows": med["bucketed"] / med["rows"], "docs_per_s": {"bucketed": n / med["bucketed"] * 1e3, "rows": n / med["rows"] * 1e3}}
        del outs, r_rows, r_mask, d_src, d_dst
        torch.cuda.empty_cache()
    bf.free_model(h)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
