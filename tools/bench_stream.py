"""MEASUREMENT: the stream stage (IdsToStreamRowsBatchDevice: ragged ids -> [R, L] rows cut from the stream of all sequences, with segment ids,
position ids and next-token labels) beside the packed stage on the same ids at the same L and a plain copy.

Two inputs, each tokenised once (TextToIdsBatchDevice, untruncated); the ids stay resident on the device:
  config2   `--docs` documents of bfutil.gen_corpus (workload config2) under bert_base_tok.bin ([CLS] / [SEP]), at L = 128 and L = 512
  config3   `--docs3` documents of workload config3 (32 .. 2048 bytes) under gpt2.bin (no leading special, <|endoftext|> behind), at L = 1024
Every output of the stream stage -- the four planes, the row-first pair, the per-sequence pair, {R, T} -- is verified first against the
vectorised restatement of the specification (tests/stream_cases.py restate_np; the CPU tier holds it to the sequential one) applied to the same
ids.  Then four things are timed in this process, in alternating windows of at least `--window-seconds` each (device events around a window,
calls back to back on one stream with one synchronisation per 8 calls, a warm-up call of each before the first window), median of `--windows`
windows with the spread:

  stream         (a) IdsToStreamRowsBatchDevice with rows, seg and pos (and the per-sequence outputs), rows_cap = R
  stream_labels  (b) the same with labels
  packed         (c) IdsToPackedRowsBatchDevice on the same ids and L with every output, rows_cap = its R
  copy           (d) one hipMemcpyAsync, device to device, of as many bytes as (a) writes

and, from the events the stream call records on its stream (BfLastKernelMs, median of 21 synchronised calls): widths + scan, the per-sequence
outputs, the fill.  The bar: (a) takes no longer than (c) plus the spread (max - min) of (c) measured in this command; (a)/(d) and (b)/(a) are
recorded.  Writes profiles/stream_bench.json.

  python tools/bench_stream.py [--docs 1000000] [--docs3 1000000] [--windows 5] [--out profiles/stream_bench.json]"""
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
    ap.add_argument("--docs3", type=int, default=1000000)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--window-seconds", type=float, default=1.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_bench.json"))
    a = ap.parse_args()

    import torch
    import bfutil
    import blingfire_amd as bf
    import stream_cases as sc

    if not torch.cuda.is_available():
        sys.exit("bench_stream.py measures on the GPU: no device is visible")
    VP = ctypes.c_void_p
    IGN = -100
    lib = bf.lib()
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream()
    sp = VP(stream.cuda_stream)
    hip = ctypes.CDLL("libamdhip64.so")                         # the HIP runtime torch and the library already run on
    hip.hipMemcpyAsync.restype = ctypes.c_int
    hip.hipMemcpyAsync.argtypes = [VP, VP, ctypes.c_size_t, ctypes.c_int, VP]

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

    res = {"device": torch.cuda.get_device_name(0), "window_seconds": a.window_seconds, "verified": True, "cases": []}
    for workload, model, n, bos, eos, pad, unk, row_lens in (("config2", "bert_base_tok.bin", a.docs, 101, 102, 0, 100, (128, 512)),
                                                             ("config3", "gpt2.bin", a.docs3, -1, 50256, 50256, 0, (1024,))):
        if n <= 0:
            continue
        text, off = bfutil.gen_corpus(n, **bfutil.WORKLOADS[workload]["gen"])
        total = int(off[-1])
        h = bf.load_model(bfutil.model_path(model))
        d_text, d_off = torch.from_numpy(text).to(dev), torch.from_numpy(off).to(dev)
        assert lib.BfReserve(VP(h), n, total, 0) == 0
        ids_cap = total + n + 1                                 # (neither model yields more ids than bytes)
        d_ids = torch.empty(ids_cap, dtype=torch.int32, device=dev)
        d_idoff = torch.empty(n + 1, dtype=torch.int64, device=dev)
        assert lib.TextToIdsBatchDevice(VP(h), d_text.data_ptr(), d_off.data_ptr(), n, total, d_ids.data_ptr(), ids_cap, d_idoff.data_ptr(), 0x7fffffff, unk, sp) == 0
        torch.cuda.synchronize()
        assert lib.BfLastStatus(VP(h)) == 0
        idoff_h = d_idoff.cpu().numpy()
        nids = int(idoff_h[-1])
        ids_h = d_ids.cpu().numpy()[:nids]
        del d_text, text
        for L in row_lens:
            d_nrows = torch.zeros(2, dtype=torch.int64, device=dev)
            pre = (VP(h), d_ids.data_ptr(), ids_cap, d_idoff.data_ptr(), n, L, bos, eos, pad, IGN, 0)
            assert lib.IdsToStreamRowsBatchDevice(*pre, *[None] * 6, 0, None, None, d_nrows.data_ptr(), sp) == 0            # the size query
            R, T = d_nrows.tolist()
            planes = [torch.empty((R, L), dtype=torch.int32, device=dev) for _ in range(4)]
            d_first = [torch.empty(R, dtype=torch.int32, device=dev) for _ in range(2)]
            d_seq = [torch.empty(n, dtype=torch.int32, device=dev) for _ in range(2)]
            stream_bytes = 3 * R * L * 4 + 2 * n * 4 + 16
            p_nrows = torch.zeros(1, dtype=torch.int64, device=dev)
            ppre = (VP(h), d_ids.data_ptr(), ids_cap, d_idoff.data_ptr(), n, L, bos, eos, pad, 0)
            assert lib.IdsToPackedRowsBatchDevice(*ppre, None, None, None, None, 0, None, None, p_nrows.data_ptr(), sp) == 0
            PR = int(p_nrows.item())
            p_planes = [torch.empty((PR, L), dtype=torch.int32, device=dev) for _ in range(3)]
            p_first = torch.empty(PR + 1, dtype=torch.int32, device=dev)
            p_seq = [torch.empty(n, dtype=torch.int32, device=dev) for _ in range(2)]
            packed_bytes = 3 * PR * L * 4 + (PR + 1) * 4 + 2 * n * 4 + 8
            d_src = torch.zeros(stream_bytes, dtype=torch.uint8, device=dev)
            d_dst = torch.empty(stream_bytes, dtype=torch.uint8, device=dev)

            def run_stream(labels, firsts):
                r = lib.IdsToStreamRowsBatchDevice(*pre, planes[0].data_ptr(), planes[1].data_ptr(), planes[2].data_ptr(), planes[3].data_ptr() if labels else None,
                                                   d_first[0].data_ptr() if firsts else None, d_first[1].data_ptr() if firsts else None, R,
                                                   d_seq[0].data_ptr(), d_seq[1].data_ptr(), d_nrows.data_ptr(), sp)
                assert r == 0, r

            def stream_a():
                run_stream(False, False)

            def stream_b():
                run_stream(True, False)

            def packed():
                r = lib.IdsToPackedRowsBatchDevice(*ppre, p_planes[0].data_ptr(), p_planes[1].data_ptr(), p_planes[2].data_ptr(), p_first.data_ptr(), PR,
                                                   p_seq[0].data_ptr(), p_seq[1].data_ptr(), p_nrows.data_ptr(), sp)
                assert r == 0, r

            def copy():
                r = hip.hipMemcpyAsync(d_dst.data_ptr(), d_src.data_ptr(), stream_bytes, 3, sp)      # 3 = hipMemcpyDeviceToDevice
                assert r == 0, r

            # warm-up, and the run that is verified: every output, labels and the row-first pair included
            run_stream(True, True); packed(); copy()
            torch.cuda.synchronize()
            assert lib.BfLastStatus(VP(h)) == 0
            want = sc.restate_np(ids_h, idoff_h, L, bos, eos, pad, IGN, 0)
            assert (want[8], want[9]) == (R, T) and d_nrows.tolist() == [R, T], "the counts differ from the restatement"
            for name, got, w in zip(sc.NAMES, (*planes, *d_first, *d_seq), want):
                assert np.array_equal(got.cpu().numpy(), w), "%s differ from the restatement" % name
            del want
            for t in planes:
                t.fill_(-1)
            stream_a()
            torch.cuda.synchronize()
            assert bool((planes[3] == -1).all().item()) and bool((planes[0] != -1).all().item()), "(a) must leave the labels alone and write the rows"

            stages = []
            buf = (ctypes.c_float * 6)()
            for _ in range(21):
                stream_a()
                assert lib.BfLastKernelMs(VP(h), buf, 6) == 6
                stages.append([buf[i] for i in range(6)])
            st = [statistics.median(s[i] for s in stages) for i in range(6)]

            times = {"stream": [], "stream_labels": [], "packed": [], "copy": []}
            for _ in range(a.windows):
                for name, fn in (("stream", stream_a), ("stream_labels", stream_b), ("packed", packed), ("copy", copy)):
                    times[name].append(window(fn))
            med = {k: statistics.median(v) for k, v in times.items()}
            spread_c = max(times["packed"]) - min(times["packed"])
            res["cases"].append({
                "workload": workload, "model": model, "docs": n, "text_bytes": total, "ids": nids, "row_len": L, "stream_rows": R, "stream_len": T, "packed_rows": PR,
                "stream": summary(times["stream"]), "stream_labels": summary(times["stream_labels"]), "packed": summary(times["packed"]), "copy": summary(times["copy"]),
                "stream_stages_ms": {"widths_scan": st[0], "seq_outputs": st[2], "fill": st[3], "total": st[4]},
                "stream_bytes_written": stream_bytes, "packed_bytes_written": packed_bytes,
                "bar": {"stream_median_ms": med["stream"], "packed_median_ms": med["packed"], "packed_spread_ms": spread_c, "met": med["stream"] <= med["packed"] + spread_c},
                "stream_over_copy": med["stream"] / med["copy"], "labels_over_stream": med["stream_labels"] / med["stream"],
                "stream_written_GBps": stream_bytes / med["stream"] / 1e6, "copy_GBps": stream_bytes / med["copy"] / 1e6})
            del planes, p_planes, d_src, d_dst
            torch.cuda.empty_cache()
        bf.free_model(h)
        del d_ids
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
