"""MEASUREMENT: MLM masking of rows on the device (RowsMlmMaskBatchDevice, k_rows_mlm), token form and whole-word form, beside a plain copy of
the bytes the call writes.

1 M documents of bfutil.gen_corpus (workload config2) under bert_base_tok.bin are tokenised once on the device with offsets (max_len = 62) and
laid out as rows of L = 64 with [CLS] / [SEP], a mask and the two offset planes (IdsToRowsPlanesBatchDevice, fill -1).  Both forms mask with
select 0.15, mask 0.8, random 0.1, the specials [CLS] [SEP] [PAD], and write both outputs (ids out of place, labels).  Every cell of both outputs
of both forms is verified first against the restatement of tests/mlm_cases.py (the array form of the heads, which is held to the loop of the
definition on a sample of the rows).

Timed in this process in alternating windows of at least one second each (device events around a window, calls back to back on one stream, a
warm-up call of each before the first window), median of `--windows` windows with the spread:

  mlm_token         RowsMlmMaskBatchDevice without offset planes: k_rows_mlm<64, false>
  mlm_whole_word    the same with the two planes: k_rows_mlm<64, true>
  mlm_copy          one hipMemcpyAsync, device to device, of the bytes the call writes (two [rows, 64] int32 outputs)

The call is the status-word clear and one kernel, so a call's time is the kernel's.  Writes profiles/mlm_bench.json.

  python tools/bench_mlm.py [--docs 1000000] [--windows 5] [--out profiles/mlm_bench.json]"""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mlm_bench.json"))
    a = ap.parse_args()

    import torch
    import bfutil
    import blingfire_amd as bf
    import mlm_cases as mc

    if not torch.cuda.is_available():
        sys.exit("bench_mlm.py measures on the GPU: no device is visible")
    VP, I32 = ctypes.c_void_p, ctypes.c_int32
    L, CLS, SEP, PAD, MASK, UNK = 64, 101, 102, 0, 103, 100
    PROBS, RAND, SEED, EPOCH = (0.15, 0.8, 0.1), (1000, 30522), 20240202, 1
    wl = bfutil.WORKLOADS["config2"]
    n = a.docs
    text, off = bfutil.gen_corpus(n, **wl["gen"])
    total = int(off[-1])
    lib = bf.lib()
    h = bf.load_model(bfutil.model_path("bert_base_tok.bin"))
    dev = torch.device("cuda:0")
    d_text, d_off = torch.from_numpy(text).to(dev), torch.from_numpy(off).to(dev)
    max_len = L - 2
    ids_cap = n * max_len
    d_ids, d_st, d_en = (torch.empty(ids_cap, dtype=torch.int32, device=dev) for _ in range(3))
    d_idoff = torch.empty(n + 1, dtype=torch.int64, device=dev)
    d_rows, d_S, d_E, d_out, d_lab = (torch.empty((n, L), dtype=torch.int32, device=dev) for _ in range(5))
    d_mask = torch.empty((n, L), dtype=torch.uint8, device=dev)
    d_roff = torch.empty(n + 1, dtype=torch.int64, device=dev)
    out_bytes = 2 * n * L * 4
    d_src = torch.zeros(out_bytes, dtype=torch.uint8, device=dev)
    d_dst = torch.empty(out_bytes, dtype=torch.uint8, device=dev)
    assert lib.BfReserve(VP(h), n, total, 1) == 0
    stream = torch.cuda.current_stream()
    sp = VP(stream.cuda_stream)
    hip = ctypes.CDLL("libamdhip64.so")                         # the HIP runtime torch and the library already run on
    hip.hipMemcpyAsync.restype = ctypes.c_int
    hip.hipMemcpyAsync.argtypes = [VP, VP, ctypes.c_size_t, ctypes.c_int, VP]
    p = lambda t: t.data_ptr()                                                               # noqa: E731

    r = lib.TextToIdsWithOffsetsBatchDevice(VP(h), p(d_text), p(d_off), n, total, p(d_ids), p(d_st), p(d_en), ids_cap, p(d_idoff), max_len, UNK, sp)
    assert r == 0, r
    c_src, c_fill, c_out = (VP * 2)(p(d_st), p(d_en)), (I32 * 2)(-1, -1), (VP * 2)(p(d_S), p(d_E))
    r = lib.IdsToRowsPlanesBatchDevice(VP(h), p(d_ids), ids_cap, p(d_idoff), n, L, CLS, SEP, PAD, 0, 1, 0, p(d_rows), p(d_mask), None, None, n, p(d_roff), 2, c_src, c_fill,
                                       c_out, sp)
    assert r == 0, r
    torch.cuda.synchronize()
    assert lib.BfLastStatus(VP(h)) == 0
    c_special = (I32 * 3)(CLS, SEP, PAD)

    def mlm(whole_word):
        r = lib.RowsMlmMaskBatchDevice(VP(h), p(d_rows), L, n, d_roff.data_ptr() + 8 * n, p(d_mask), None, p(d_S) if whole_word else None, p(d_E) if whole_word else None,
                                       3, c_special, *PROBS, MASK, RAND[0], RAND[1], -100, SEED, EPOCH, p(d_out), p(d_lab), sp)
        assert r == 0, r

    def copy():
        r = hip.hipMemcpyAsync(p(d_dst), p(d_src), out_bytes, 3, sp)                         # 3 = hipMemcpyDeviceToDevice
        assert r == 0, r

    # ---- verification of every cell of both forms, in slices of rows on the host's threads (numpy releases the interpreter lock in its loops)
    rows_h, mask_h, S_h, E_h = d_rows.cpu().numpy(), d_mask.cpu().numpy(), d_S.cpu().numpy(), d_E.cpu().numpy()
    STEP = 1 << 14
    shares = {}
    for whole_word in (False, True):
        d_out.fill_(-7); d_lab.fill_(-7)
        mlm(whole_word)
        torch.cuda.synchronize()
        assert lib.BfLastStatus(VP(h)) == 0
        got_ids, got_lab = d_out.cpu().numpy(), d_lab.cpu().numpy()

        def verify(b):
            e = min(n, b + STEP)
            want = mc.restate_mlm(rows_h[b:e], mask_h[b:e], None, S_h[b:e] if whole_word else None, E_h[b:e] if whole_word else None, special_ids=[CLS, SEP, PAD],
                                  probs=PROBS, mask_id=MASK, rand_range=RAND, seed=SEED, epoch=EPOCH, row_base=b, heads_fn=mc.heads_array)
            return np.array_equal(got_ids[b:e], want[0]) and np.array_equal(got_lab[b:e], want[1])
        with ThreadPoolExecutor(max_workers=min(16, bfutil.host_threads())) as pool:
            assert all(pool.map(verify, range(0, n, STEP))), "%s form differs from the restatement" % ("whole-word" if whole_word else "token")
        el = mc.eligible(rows_h, mask_h, None, [CLS, SEP, PAD])
        sel = got_lab != -100
        shares["whole_word" if whole_word else "token"] = {"eligible_cells": int(el.sum()), "selected_share_of_eligible": float(sel.sum() / max(int(el.sum()), 1)),
                                                            "mask_share_of_selected": float((got_ids[sel] == MASK).mean()) if sel.any() else 0.0}
    k = min(n, 512)
    el_k = mc.eligible(rows_h[:k], mask_h[:k], None, [CLS, SEP, PAD])
    hd = mc.heads(el_k, S_h[:k], E_h[:k])
    assert np.array_equal(hd, mc.heads_array(el_k, S_h[:k], E_h[:k])), "the array form of the heads differs from the loop"
    cells_in_units = float((mc.heads_array(el, S_h, E_h) != np.arange(L)[None, :]).sum() / max(int(el.sum()), 1))
    del rows_h, mask_h, S_h, E_h, got_ids, got_lab, el, sel

    fns = [("mlm_token", lambda: mlm(False)), ("mlm_whole_word", lambda: mlm(True)), ("mlm_copy", copy)]
    for _, fn in fns:
        fn()
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

    times = {name: [] for name, _ in fns}
    for _ in range(a.windows):
        for name, fn in fns:
            times[name].append(window(fn))
    bf.free_model(h)

    def summary(v):
        return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "windows": len(v)}
    med = {name: statistics.median(v) for name, v in times.items()}
    read_token, read_ww = n * L * 5, n * L * 13                                              # ids + mask byte; + two offset planes
    res = {"docs": n, "rows": n, "row_len": L, "text_bytes": total, "model": "bert_base_tok.bin", "workload": "config2", "max_len": max_len, "probabilities": list(PROBS),
           "verified": True, "shares": shares, "continuing_share_of_eligible_cells": cells_in_units, "device": torch.cuda.get_device_name(0),
           "window_seconds": a.window_seconds, "bytes_written": out_bytes, "bytes_read_token": read_token, "bytes_read_whole_word": read_ww}
    for name in times:
        res[name] = summary(times[name])
    res.update({"mlm_token_over_copy": med["mlm_token"] / med["mlm_copy"], "mlm_whole_word_over_copy": med["mlm_whole_word"] / med["mlm_copy"],
                "mlm_whole_word_over_token": med["mlm_whole_word"] / med["mlm_token"],
                "mlm_token_moved_GBps": (read_token + out_bytes) / med["mlm_token"] / 1e6, "mlm_whole_word_moved_GBps": (read_ww + out_bytes) / med["mlm_whole_word"] / 1e6,
                "mlm_copy_written_GBps": out_bytes / med["mlm_copy"] / 1e6, "mlm_token_cells_per_us": n * L / med["mlm_token"] / 1e3})
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
