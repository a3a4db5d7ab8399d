"""MEASUREMENT: the span-corruption call (RowsDenoiseBatchDevice, k_rows_denoise) beside the MLM call (RowsMlmMaskBatchDevice, k_rows_mlm, token by
token) on the same rows in the same process, and beside a plain copy of the bytes the new call writes.

Two shapes: stream rows of L = 128 and of L = 512.  For each, 1 M documents of bfutil.gen_corpus (workload config2) under bert_base_tok.bin are
tokenised once on the device and laid end to end as stream rows with [SEP] behind every document (IdsToStreamRowsBatchDevice: rows and the segment
plane; its row count bounds the rows of every timed call).  The spec is start_prob = denoise_start_prob(0.15, 1, 5), lengths 1 .. 5, 100 sentinels
downwards from the end of the vocabulary, the specials [SEP] [PAD], enc_len = L, dec_len = L + 2.  Every entry of all seven outputs is verified first
against the array form of the restatement of tests/denoise_cases.py, which is held to the loop of the definition on the first rows.

Timed in alternating windows of at least one second each (device events around a window, calls back to back on one stream, a warm-up call of each
before the first window), median of `--windows` windows with the spread:

  denoise            RowsDenoiseBatchDevice, the two id planes and the three counts
  denoise_cells      the same with the two source-cell planes
  mlm_token          RowsMlmMaskBatchDevice on the same rows (ids and labels out of place): one walk, one Philox evaluation per cell -- the yardstick
  copy / copy_cells  one hipMemcpyAsync, device to device, of the bytes `denoise` / `denoise_cells` writes

Either call is the status-word clear and one kernel, so a call's time is the kernel's.  Writes profiles/denoise_bench.json.

  python tools/bench_denoise.py [--docs 1000000] [--windows 5] [--out profiles/denoise_bench.json]"""
import argparse
import ctypes
import json
import os
import statistics
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1000000)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--window-seconds", type=float, default=1.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "denoise_bench.json"))
    a = ap.parse_args()

    import torch
    import bfutil
    import blingfire_amd as bf
    import denoise_cases as dc

    if not torch.cuda.is_available():
        sys.exit("bench_denoise.py measures on the GPU: no device is visible")
    VP, I32 = ctypes.c_void_p, ctypes.c_int32
    SEP, PAD, MASK, UNK = 102, 0, 103, 100
    SEED, EPOCH = 20240303, 1
    SPECIALS = [SEP, PAD]
    SPEC = dict(special_ids=SPECIALS, start_prob=bf.denoise_start_prob(0.15, 1, 5), len_lo=1, len_hi=5, sentinel_first=30521, sentinel_step=-1, max_sentinels=100,
                eos_id=SEP, pad_id=PAD, ignore_label=-100, seed=SEED, epoch=EPOCH)
    wl = bfutil.WORKLOADS["config2"]
    n = a.docs
    text, off = bfutil.gen_corpus(n, **wl["gen"])
    total = int(off[-1])
    lib = bf.lib()
    h = bf.load_model(bfutil.model_path("bert_base_tok.bin"))
    dev = torch.device("cuda:0")
    d_text, d_off = torch.from_numpy(text).to(dev), torch.from_numpy(off).to(dev)
    stream = torch.cuda.current_stream()
    sp = VP(stream.cuda_stream)
    hip = ctypes.CDLL("libamdhip64.so")                         # the HIP runtime torch and the library already run on
    hip.hipMemcpyAsync.restype = ctypes.c_int
    hip.hipMemcpyAsync.argtypes = [VP, VP, ctypes.c_size_t, ctypes.c_int, VP]
    p = lambda t: t.data_ptr()                                                               # noqa: E731
    c_special = (I32 * 2)(*SPECIALS)
    d_ids, d_idoff = bf.text_to_ids_batch_device(h, d_text, d_off, 0x7fffffff, UNK)
    torch.cuda.synchronize()
    assert lib.BfLastStatus(VP(h)) == 0
    d_ids = d_ids[:int(d_idoff[-1].item())]                     # (the ids there are, not the buffer's capacity: the row calls size their outputs by it)

    def summary(v):
        return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "windows": len(v)}

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

    res = {"docs": n, "text_bytes": total, "model": "bert_base_tok.bin", "workload": "config2", "noise_density": 0.15, "start_prob": SPEC["start_prob"],
           "lengths": [1, 5], "verified": True, "device": torch.cuda.get_device_name(0), "window_seconds": a.window_seconds, "shapes": {}}
    for L in (128, 512):
        got = bf.ids_to_stream_rows_batch_device(h, d_ids, d_idoff, L, None, SEP, PAD)
        d_rows, d_seg, d_nrows = got[0], got[1], got[8]
        torch.cuda.synchronize()
        assert lib.BfLastStatus(VP(h)) == 0
        R, T = int(d_nrows[0].item()), int(d_nrows[1].item())
        cap = d_rows.shape[0]
        del got
        EL, DL = L, L + 2
        d_enc, d_ecell = (torch.empty((cap, EL), dtype=torch.int32, device=dev) for _ in range(2))
        d_dec, d_dcell = (torch.empty((cap, DL), dtype=torch.int32, device=dev) for _ in range(2))
        d_cnt = [torch.empty((cap,), dtype=torch.int32, device=dev) for _ in range(3)]
        d_out, d_lab = (torch.empty((cap, L), dtype=torch.int32, device=dev) for _ in range(2))
        out_bytes = R * (EL + DL + 3) * 4
        out_bytes_cells = R * (2 * EL + 2 * DL + 3) * 4
        d_src = torch.zeros(out_bytes_cells, dtype=torch.uint8, device=dev)
        d_dst = torch.empty(out_bytes_cells, dtype=torch.uint8, device=dev)
        print("L = %d: %d rows laid out (%d cells of the stream)" % (L, R, T), file=sys.stderr, flush=True)

        def denoise(cells):
            r = lib.RowsDenoiseBatchDevice(VP(h), p(d_rows), L, cap, p(d_nrows), None, p(d_seg), 2, c_special, SPEC["start_prob"], 1, 5, SPEC["sentinel_first"], -1, 100, SEP, PAD,
                                           -100, SEED, EPOCH, EL, p(d_enc), p(d_ecell) if cells else None, p(d_cnt[0]), DL, p(d_dec), p(d_dcell) if cells else None, p(d_cnt[1]),
                                           p(d_cnt[2]), sp)
            assert r == 0, r

        def mlm():
            r = lib.RowsMlmMaskBatchDevice(VP(h), p(d_rows), L, cap, p(d_nrows), None, p(d_seg), None, None, 2, c_special, 0.15, 0.8, 0.1, MASK, 1000, 30522, -100, SEED, EPOCH,
                                           p(d_out), p(d_lab), sp)
            assert r == 0, r

        def copy(nbytes):
            r = hip.hipMemcpyAsync(p(d_dst), p(d_src), nbytes, 3, sp)                        # 3 = hipMemcpyDeviceToDevice
            assert r == 0, r

        # ---- verification of every entry of the seven outputs, in slices of rows on the host's threads
        outs = dict(enc=d_enc, enc_cell=d_ecell, enc_count=d_cnt[0], dec=d_dec, dec_cell=d_dcell, dec_count=d_cnt[1], span_count=d_cnt[2])
        for t in outs.values():
            t.fill_(-7)
        denoise(True)
        torch.cuda.synchronize()
        assert lib.BfLastStatus(VP(h)) == 0
        got = {k: t.cpu().numpy()[:R] for k, t in outs.items()}
        assert all(bool((t[R:] == -7).all()) for t in outs.values()), "a row at or past the row count was written"
        rows_h, seg_h = d_rows.cpu().numpy()[:R], d_seg.cpu().numpy()[:R]
        STEP = max(1, (1 << 21) // L)

        def verify(b):
            e = min(R, b + STEP)
            want = dc.restate_denoise(rows_h[b:e], None, seg_h[b:e], row_base=b, array=True, **SPEC)
            return all(np.array_equal(got[k][b:e], want[k]) for k in dc.NAMES), int(want["noise"].sum()), int(want["span_count"].sum()), int(want["eligible"].sum())
        with ThreadPoolExecutor(max_workers=min(16, bfutil.host_threads())) as pool:
            parts = list(pool.map(verify, range(0, R, STEP)))
        assert all(x[0] for x in parts), "L = %d differs from the restatement" % L
        k = min(R, 256)
        loop = dc.restate_denoise(rows_h[:k], None, seg_h[:k], **SPEC)
        assert all(np.array_equal(got[name][:k], loop[name]) for name in dc.NAMES), "the array form of the restatement differs from the loop"
        print("L = %d: verified" % L, file=sys.stderr, flush=True)
        shares = {"noise_cells_of_eligible": sum(x[1] for x in parts) / max(1, sum(x[3] for x in parts)), "spans_per_row": sum(x[2] for x in parts) / R,
                  "eligible_cells_per_row": sum(x[3] for x in parts) / R}
        del rows_h, seg_h, got

        fns = [("denoise", lambda: denoise(False)), ("mlm_token", mlm), ("copy", lambda: copy(out_bytes)), ("denoise_cells", lambda: denoise(True)),
               ("copy_cells", lambda: copy(out_bytes_cells))]
        for _, fn in fns:
            fn()
        torch.cuda.synchronize()
        times = {name: [] for name, _ in fns}
        for _ in range(a.windows):
            for name, fn in fns:
                times[name].append(window(fn))
        med = {name: statistics.median(v) for name, v in times.items()}
        shape = {"row_len": L, "rows": R, "stream_cells": T, "enc_len": EL, "dec_len": DL, "shares": shares, "bytes_read": R * L * 8, "bytes_written": out_bytes,
                 "bytes_written_cells": out_bytes_cells, "bytes_written_mlm": 2 * R * L * 4}
        for name in times:
            shape[name] = summary(times[name])
        shape.update({"denoise_over_mlm_token": med["denoise"] / med["mlm_token"], "denoise_cells_over_mlm_token": med["denoise_cells"] / med["mlm_token"],
                      "denoise_over_copy": med["denoise"] / med["copy"], "denoise_cells_over_copy": med["denoise_cells"] / med["copy_cells"],
                      "denoise_cells_per_us": R * L / med["denoise"] / 1e3, "mlm_token_cells_per_us": R * L / med["mlm_token"] / 1e3,
                      "denoise_gb_per_s": (R * L * 8 + out_bytes) / med["denoise"] / 1e6})
        res["shapes"]["L%d" % L] = shape
        del d_rows, d_seg, d_enc, d_ecell, d_dec, d_dcell, d_cnt, d_out, d_lab, d_src, d_dst, outs
        torch.cuda.empty_cache()
    bf.free_model(h)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
