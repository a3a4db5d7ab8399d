"""MEASUREMENT: the capped MLM call (RowsMlmPredictionsBatchDevice, k_rows_mlm_cap) beside the base call (RowsMlmMaskBatchDevice, k_rows_mlm) on the
same rows in the same process, and beside a plain copy of the bytes the new call writes.

Two shapes: rows of L = 64 with P = 10 predictions and rows of L = 128 with P = 20 (max_predictions_per_seq of the BERT data pipeline at 128).  For
each, 1 M documents of bfutil.gen_corpus (workload config2) under bert_base_tok.bin are tokenised once on the device with offsets (max_len = L - 2)
and laid out as rows with [CLS] / [SEP], a mask and the two offset planes (IdsToRowsPlanesBatchDevice, fill -1).  Token form and whole-word form mask
with select 0.15, mask 0.8, random 0.1, the specials [CLS] [SEP] [PAD], and write all five outputs (ids out of place).  Every entry of all five
outputs of both forms is verified first against the array form of the restatement of tests/mlmcap_cases.py, which is held to the loop of the
definition on the first rows.

Timed in alternating windows of at least one second each (device events around a window, calls back to back on one stream, a warm-up call of each
before the first window), median of `--windows` windows with the spread:

  cap_token / cap_whole_word      RowsMlmPredictionsBatchDevice with max_pred = P: k_rows_mlm_cap<64, false / true, C>
  base_token / base_whole_word    RowsMlmMaskBatchDevice on the same rows: k_rows_mlm<64, false / true>
  cap_copy                        one hipMemcpyAsync, device to device, of the bytes the new call writes
  *_select50                      the four calls again with select 0.5 (also verified): the documents of config 2 are short, so at 0.15 the cap binds in
                                  few rows and the threshold search hardly runs; at 0.5 it runs in most rows

Either call is the status-word clear and one kernel, so a call's time is the kernel's.  Writes profiles/mlmcap_bench.json.

  python tools/bench_mlmcap.py [--docs 1000000] [--windows 5] [--out profiles/mlmcap_bench.json]"""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mlmcap_bench.json"))
    a = ap.parse_args()

    import torch
    import bfutil
    import blingfire_amd as bf
    import mlm_cases as mc
    import mlmcap_cases as cc

    if not torch.cuda.is_available():
        sys.exit("bench_mlmcap.py measures on the GPU: no device is visible")
    VP, I32 = ctypes.c_void_p, ctypes.c_int32
    CLS, SEP, PAD, MASK, UNK = 101, 102, 0, 103, 100
    PROBS, RAND, SEED, EPOCH = (0.15, 0.8, 0.1), (1000, 30522), 20240202, 1
    DENSE = (0.5, 0.8, 0.1)                                    # the documents of config 2 are short: at 0.15 the cap rarely binds, at 0.5 it does in most rows
    SPECIALS = [CLS, SEP, PAD]
    wl = bfutil.WORKLOADS["config2"]
    n = a.docs
    text, off = bfutil.gen_corpus(n, **wl["gen"])
    total = int(off[-1])
    lib = bf.lib()
    h = bf.load_model(bfutil.model_path("bert_base_tok.bin"))
    dev = torch.device("cuda:0")
    d_text, d_off = torch.from_numpy(text).to(dev), torch.from_numpy(off).to(dev)
    assert lib.BfReserve(VP(h), n, total, 1) == 0
    stream = torch.cuda.current_stream()
    sp = VP(stream.cuda_stream)
    hip = ctypes.CDLL("libamdhip64.so")                         # the HIP runtime torch and the library already run on
    hip.hipMemcpyAsync.restype = ctypes.c_int
    hip.hipMemcpyAsync.argtypes = [VP, VP, ctypes.c_size_t, ctypes.c_int, VP]
    p = lambda t: t.data_ptr()                                                               # noqa: E731
    c_special = (I32 * 3)(*SPECIALS)

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

    res = {"docs": n, "rows": n, "text_bytes": total, "model": "bert_base_tok.bin", "workload": "config2", "probabilities": list(PROBS), "verified": True,
           "device": torch.cuda.get_device_name(0), "window_seconds": a.window_seconds, "shapes": {}}
    for L, P in ((64, 10), (128, 20)):
        max_len = L - 2
        ids_cap = n * max_len
        d_ids, d_st, d_en = (torch.empty(ids_cap, dtype=torch.int32, device=dev) for _ in range(3))
        d_idoff = torch.empty(n + 1, dtype=torch.int64, device=dev)
        d_rows, d_S, d_E, d_out, d_lab = (torch.empty((n, L), dtype=torch.int32, device=dev) for _ in range(5))
        d_cell, d_plab = (torch.empty((n, P), dtype=torch.int32, device=dev) for _ in range(2))
        d_cnt = torch.empty((n,), dtype=torch.int32, device=dev)
        d_mask = torch.empty((n, L), dtype=torch.uint8, device=dev)
        d_roff = torch.empty(n + 1, dtype=torch.int64, device=dev)
        out_bytes = 2 * n * L * 4 + 2 * n * P * 4 + n * 4
        d_src = torch.zeros(out_bytes, dtype=torch.uint8, device=dev)
        d_dst = torch.empty(out_bytes, dtype=torch.uint8, device=dev)
        r = lib.TextToIdsWithOffsetsBatchDevice(VP(h), p(d_text), p(d_off), n, total, p(d_ids), p(d_st), p(d_en), ids_cap, p(d_idoff), max_len, UNK, sp)
        assert r == 0, r
        c_src, c_fill, c_out = (VP * 2)(p(d_st), p(d_en)), (I32 * 2)(-1, -1), (VP * 2)(p(d_S), p(d_E))
        r = lib.IdsToRowsPlanesBatchDevice(VP(h), p(d_ids), ids_cap, p(d_idoff), n, L, CLS, SEP, PAD, 0, 1, 0, p(d_rows), p(d_mask), None, None, n, p(d_roff), 2, c_src,
                                           c_fill, c_out, sp)
        assert r == 0, r
        torch.cuda.synchronize()
        assert lib.BfLastStatus(VP(h)) == 0
        del d_ids, d_st, d_en
        print("L = %d: rows laid out" % L, file=sys.stderr, flush=True)

        def head(whole_word, probs):
            return (VP(h), p(d_rows), L, n, d_roff.data_ptr() + 8 * n, p(d_mask), None, p(d_S) if whole_word else None, p(d_E) if whole_word else None, 3, c_special, *probs,
                    MASK, RAND[0], RAND[1], -100, SEED, EPOCH, p(d_out), p(d_lab))

        def cap(whole_word, probs=PROBS):
            r = lib.RowsMlmPredictionsBatchDevice(*head(whole_word, probs), P, p(d_cell), p(d_plab), p(d_cnt), sp)
            assert r == 0, r

        def base(whole_word, probs=PROBS):
            r = lib.RowsMlmMaskBatchDevice(*head(whole_word, probs), sp)
            assert r == 0, r

        def copy():
            r = hip.hipMemcpyAsync(p(d_dst), p(d_src), out_bytes, 3, sp)                     # 3 = hipMemcpyDeviceToDevice
            assert r == 0, r

        # ---- verification of every entry of the five outputs of both forms, in slices of rows on the host's threads
        rows_h, mask_h, S_h, E_h = d_rows.cpu().numpy(), d_mask.cpu().numpy(), d_S.cpu().numpy(), d_E.cpu().numpy()
        STEP = 1 << 14
        shares = {}
        for whole_word, probs in ((False, PROBS), (True, PROBS), (False, DENSE), (True, DENSE)):
            for t in (d_out, d_lab, d_cell, d_plab, d_cnt):
                t.fill_(-7)
            cap(whole_word, probs)
            torch.cuda.synchronize()
            assert lib.BfLastStatus(VP(h)) == 0
            got = [t.cpu().numpy() for t in (d_out, d_lab, d_cell, d_plab, d_cnt)]
            planes = (S_h, E_h) if whole_word else (None, None)
            kw = dict(special_ids=SPECIALS, probs=probs, mask_id=MASK, rand_range=RAND, seed=SEED, epoch=EPOCH, max_pred=P)

            def verify(b):
                e = min(n, b + STEP)
                want = cc.restate_cap(rows_h[b:e], mask_h[b:e], None, *[None if x is None else x[b:e] for x in planes], row_base=b, heads_fn=mc.heads_array,
                                      kept_fn=cc.kept_array, **kw)
                uncapped = mc.restate_mlm(rows_h[b:e], mask_h[b:e], None, *[None if x is None else x[b:e] for x in planes], special_ids=SPECIALS, probs=probs, mask_id=MASK,
                                          rand_range=RAND, seed=SEED, epoch=EPOCH, row_base=b, heads_fn=mc.heads_array)[1] != -100
                ok = all(np.array_equal(g[b:e], w) for g, w in zip(got, want))
                return ok, int((uncapped.sum(axis=1) > want[4]).sum()), int(uncapped.sum()), int(want[4].sum())
            with ThreadPoolExecutor(max_workers=min(16, bfutil.host_threads())) as pool:
                parts = list(pool.map(verify, range(0, n, STEP)))
            print("L = %d %s form, select %.2f: verified" % (L, "whole-word" if whole_word else "token", probs[0]), file=sys.stderr, flush=True)
            assert all(x[0] for x in parts), "%s form at L = %d differs from the restatement" % ("whole-word" if whole_word else "token", L)
            k = min(n, 256)
            loop = cc.restate_cap(rows_h[:k], mask_h[:k], None, *[None if x is None else x[:k] for x in planes], **kw)
            assert all(np.array_equal(g[:k], w) for g, w in zip(got, loop)), "the array form of the restatement differs from the loop"
            shares[("whole_word" if whole_word else "token") + ("" if probs is PROBS else "_select50")] = {"rows_the_cap_binds_in": sum(x[1] for x in parts) / n, "selected_cells_per_row": sum(x[2] for x in parts) / n,
                                                                "kept_cells_per_row": sum(x[3] for x in parts) / n}
        del rows_h, mask_h, S_h, E_h, got

        fns = [("cap_token", lambda: cap(False)), ("base_token", lambda: base(False)), ("cap_whole_word", lambda: cap(True)), ("base_whole_word", lambda: base(True)),
               ("cap_copy", copy), ("cap_token_select50", lambda: cap(False, DENSE)), ("base_token_select50", lambda: base(False, DENSE)),
               ("cap_whole_word_select50", lambda: cap(True, DENSE)), ("base_whole_word_select50", lambda: base(True, DENSE))]
        for _, fn in fns:
            fn()
        torch.cuda.synchronize()
        times = {name: [] for name, _ in fns}
        for _ in range(a.windows):
            for name, fn in fns:
                times[name].append(window(fn))
        med = {name: statistics.median(v) for name, v in times.items()}
        shape = {"row_len": L, "max_pred": P, "max_len": max_len, "shares": shares, "bytes_written": out_bytes, "bytes_written_base": 2 * n * L * 4,
                 "bytes_read_token": n * L * 5, "bytes_read_whole_word": n * L * 13}
        for name in times:
            shape[name] = summary(times[name])
        shape.update({"cap_token_over_base_token": med["cap_token"] / med["base_token"], "cap_whole_word_over_base_whole_word": med["cap_whole_word"] / med["base_whole_word"],
                      "cap_token_select50_over_base": med["cap_token_select50"] / med["base_token_select50"],
                      "cap_whole_word_select50_over_base": med["cap_whole_word_select50"] / med["base_whole_word_select50"],
                      "cap_token_over_copy": med["cap_token"] / med["cap_copy"], "cap_whole_word_over_copy": med["cap_whole_word"] / med["cap_copy"],
                      "cap_token_cells_per_us": n * L / med["cap_token"] / 1e3, "cap_whole_word_cells_per_us": n * L / med["cap_whole_word"] / 1e3})
        res["shapes"]["L%d_P%d" % (L, P)] = shape
        del d_rows, d_S, d_E, d_out, d_lab, d_cell, d_plab, d_cnt, d_mask, d_roff, d_src, d_dst
        torch.cuda.empty_cache()
    bf.free_model(h)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
