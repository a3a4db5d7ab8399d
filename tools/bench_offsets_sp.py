"""MEASUREMENT: the offsets step of the Unigram and BPE models (TextToIdsWithOffsetsBatchDevice) on text that is resident in HBM, beside the ids-only
step (TextToIdsBatchDevice) on the same corpus and beside the same calls under the family's baseline variant -- Unigram: BfSetVariant 6 (the
forward / backward kernels of round 4 with k_compact); BPE: 3 | 0x40 = 67 (the lane kernels with k_compact) -- in one process.

`--family unigram`: two workloads of tests/bfutil.py, config4 (xlm_roberta_base.bin) and config5 (laser500k.bin); `--family bpe`: config3
(gpt2.bin), written to profiles/offsets_bpe_bench.json; `--docs` documents each.  Before anything is
timed every id, first byte, last byte and id offset of the default call is compared with the baseline variant's on the whole corpus, and with the checker
(the compiled reference where oracle/_ref is built, else the oracle) on every `--check-step`-th document.

Timed, per variant (3 = the default, 6): a whole call in windows of at least `--window-seconds` (device events on the call's stream around a
window, calls back to back), `--windows` windows, the variants and the two calls alternating; and the per-kernel split of one call from the
events BfLastKernelMs reads (prep, tokenise, its dominant kernel, scan, compact), median of `--calls` calls.  `spread` is (max - min) / median
of a series' windows (the series' keys carry the baseline's number: ..._variant6, ..._variant67).  `--lib` times another build of the library (the parent commit's) with the same script; `--parent` merges such a run's
file into this one's and states the three comparisons: offsets and ids-only against the parent, offsets over ids-only on this build.

  python tools/bench_offsets_sp.py [--family unigram|bpe] [--docs 1000000] [--windows 7] [--calls 11] [--lib OTHER.so] [--parent PARENT.json] [--out profiles/offsets_sp_bench.json]"""
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
SEGMENTS = ("prep", "tokenise", "scan", "compact", "total", "dominant")
FAMILIES = {"unigram": (("config4", "config5"), 6, "offsets_sp_bench.json"), "bpe": (("config3",), 3 | 0x40, "offsets_bpe_bench.json")}      # workloads, baseline variant, file


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--family", choices=sorted(FAMILIES), default="unigram")
    ap.add_argument("--docs", type=int, default=1000000)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--calls", type=int, default=11)
    ap.add_argument("--check-step", type=int, default=50)
    ap.add_argument("--window-seconds", type=float, default=0.5)
    ap.add_argument("--lib", default=None)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    workloads, base, out_name = FAMILIES[a.family]
    a.out = a.out or os.path.join(ROOT, "profiles", out_name)

    import torch
    import bfutil
    import blingfire_amd as bf

    if not torch.cuda.is_available():
        sys.exit("bench_offsets_sp.py measures on the GPU: no device is visible")
    if a.lib:
        bf.LIB_PATH = os.path.abspath(a.lib)
    VP = ctypes.c_void_p
    lib = bf.lib()
    lib.BfTokeniseKernel.restype = ctypes.c_char_p; lib.BfTokeniseKernel.argtypes = [VP]
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream()
    ck, ck_name = (bfutil.reference(), "TextToIdsWithOffsets") if bfutil.have_ref() else (bfutil.oracle(), "bfo_text_to_ids_with_offsets")

    def summary(v):
        med = statistics.median(v)
        return {"median_ms": med, "min_ms": min(v), "max_ms": max(v), "n": len(v), "spread": (max(v) - min(v)) / med}

    def window(fn):
        reps = 0
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        while True:
            for _ in range(2):
                fn()
            reps += 2
            e1.record(stream)
            e1.synchronize()
            ms = e0.elapsed_time(e1)
            if ms >= a.window_seconds * 1e3:
                return ms / reps

    res = {"docs": a.docs, "library": a.lib or "this build", "device": torch.cuda.get_device_name(0), "window_seconds": a.window_seconds, "verified": True, "workloads": {}}
    for name in workloads:
        wl = bfutil.WORKLOADS[name]
        mx, unk = wl["max_ids"], wl["unk"]
        text, off = bfutil.gen_workload(name, a.docs)
        total, ndocs = int(off[-1]), len(off) - 1
        h = bf.load_model(bfutil.model_path(wl["model"]))
        d_text, d_off = torch.from_numpy(text).to(dev), torch.from_numpy(off).to(dev)
        assert lib.BfReserve(VP(h), ndocs, total, 1) == 0
        offs = lambda: bf.text_to_ids_with_offsets_batch_device(h, d_text, d_off, mx, unk)      # noqa: E731
        ids_only = lambda: bf.text_to_ids_batch_device(h, d_text, d_off, mx, unk)               # noqa: E731

        # ---- verification: the default against variant 6, every element; against the checker, every check-step-th document
        got = {}
        for v in (3, base):
            assert lib.BfSetVariant(VP(h), v) >= 0
            out = offs()
            torch.cuda.synchronize()
            assert lib.BfLastStatus(VP(h)) == 0
            got[v] = (out, lib.BfTokeniseKernel(VP(h)).decode())
        n = int(got[3][0][3][-1].item())
        assert torch.equal(got[3][0][3], got[base][0][3]) and all(torch.equal(x[:n], y[:n]) for x, y in zip(got[3][0][:3], got[base][0][:3])), (name, "the default differs from variant %d" % base)
        g_ids, g_st, g_en, g_off = (t.cpu().numpy() for t in got[3][0])
        hck = ck.load(bfutil.model_path(wl["model"]))
        raw = text.tobytes()
        checked = 0
        for d in range(0, ndocs, a.check_step):
            c, wi, ws, we = ck.with_offsets(hck, raw[off[d]:off[d + 1]], mx, unk, ck_name)
            o = int(g_off[d])
            assert c == int(g_off[d + 1]) - o and g_ids[o:o + c].tolist() == wi and g_st[o:o + c].tolist() == ws and g_en[o:o + c].tolist() == we, (name, d)
            checked += c
        ck.free(hck)
        kernels = {v: got[v][1] for v in got}
        print("%s: %d documents, %d bytes, %d tokens: equal to variant %d; %d tokens equal to the checker; kernels %s" % (name, ndocs, total, n, base, checked, kernels), file=sys.stderr, flush=True)
        del got, g_ids, g_st, g_en, raw

        # ---- timing: windows of whole calls, the series alternating; then the per-kernel split
        series = [("offsets", 3, offs), ("offsets_variant%d" % base, base, offs), ("ids", 3, ids_only), ("ids_variant%d" % base, base, ids_only)]
        times = {k: [] for k, _, _ in series}
        split = {}
        for k, v, fn in series:
            lib.BfSetVariant(VP(h), v)
            fn(); fn()
        torch.cuda.synchronize()
        for _ in range(a.windows):
            for k, v, fn in series:
                lib.BfSetVariant(VP(h), v)
                times[k].append(window(fn))
        for k, v, fn in series:
            lib.BfSetVariant(VP(h), v)
            rows = []
            for _ in range(a.calls):
                fn()
                rows.append(bf.last_kernel_ms(h))
            split[k] = {s: statistics.median(r[i] for r in rows) for i, s in enumerate(SEGMENTS[:len(rows[0])])}
        lib.BfSetVariant(VP(h), 3)
        out = {"model": wl["model"], "docs": ndocs, "text_bytes": total, "tokens": n, "max_ids": mx, "checker_tokens": checked, "kernels": kernels}
        for k in times:
            out[k] = summary(times[k])
            out[k]["kernel_ms"] = split[k]
        out["offsets_over_ids"] = out["offsets"]["median_ms"] / out["ids"]["median_ms"]
        out["offsets_over_variant%d" % base] = out["offsets"]["median_ms"] / out["offsets_variant%d" % base]["median_ms"]
        res["workloads"][name] = out
        bf.free_model(h)
        del d_text, d_off
        torch.cuda.empty_cache()
    if a.parent:
        with open(a.parent) as f:
            par = json.load(f)
        res["parent"] = {"library": par["library"], "workloads": par["workloads"]}
        for name, out in res["workloads"].items():
            p = par["workloads"][name]
            out["against_parent"] = {"parent_spread_offsets": p["offsets"]["spread"], "parent_spread_ids": p["ids"]["spread"],
                                     "offsets_over_parent": out["offsets"]["median_ms"] / p["offsets"]["median_ms"],
                                     "ids_over_parent": out["ids"]["median_ms"] / p["ids"]["median_ms"]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
