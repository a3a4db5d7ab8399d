"""MEASUREMENT: WordHyphenationBatchDevice on device-resident words against the unmodified reference's WordHyphenationWithModel on host threads.

10 M words tiled from tests/data/words_en.txt, text and offsets resident on the device.  Every word of the batch is verified first (the output
of the device call against the reference's stored answers, tiled the same way, one array comparison).  Then the device call is warmed up once
and repeated until a timed window is at least one second, device events around the window; the reference runs in the same command, whole passes
over the same words until the window is a second long, `--threads` native threads each on its own slice (tools/w2h_cpu_baseline.c through oracle/_ref).  Both rates
are the median of 5 windows, with their spread.  Writes profiles/w2h_bench.json.

  python tools/bench_w2h.py [--words 10000000] [--threads 16] [--windows 5] [--out profiles/w2h_bench.json] [--no-cpu]"""
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
    ap.add_argument("--words", type=int, default=10000000)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "w2h_bench.json"))
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--once", action="store_true", help="verify, then one device call (for a kernel trace)")
    a = ap.parse_args()

    import torch
    import bfutil
    import blingfire_amd as bf
    import secondary_cases as sc
    import w2h_cases as wc

    VP = ctypes.c_void_p
    en = wc.en_words()
    want = wc.ref_texts("batch_en", wc.FIXTURE, en)["45"]
    if len(en) % 2 == 0:
        en, want = en[:-1], want[:-1]
    idx = sc.tiling(len(en), a.words, 73)
    flat, off = sc.tile(*sc.pack(en), idx)
    w_flat, w_off = sc.tile(*wc.pack_texts(want), idx)
    n, total, T = a.words, int(off[-1]), int(w_off[-1])

    L = bf.lib()
    h = bf.load_model(wc.FIXTURE)
    dev = torch.device("cuda:0")
    d_text, d_off = torch.from_numpy(flat).to(dev), torch.from_numpy(off).to(dev)
    d_out, d_ooff = torch.zeros(T + 64, dtype=torch.uint8, device=dev), torch.zeros(n + 1, dtype=torch.int64, device=dev)
    assert L.BfReserve(VP(h), n, total, 0) == 0
    stream = torch.cuda.current_stream()

    def call():
        rc = L.WordHyphenationBatchDevice(VP(h), d_text.data_ptr(), d_off.data_ptr(), n, total, d_out.data_ptr(), T, d_ooff.data_ptr(), 0x2D, VP(stream.cuda_stream))
        assert rc == 0, rc

    call()                                                      # warm-up, and the run that is verified
    torch.cuda.synchronize()
    assert np.array_equal(d_ooff.cpu().numpy(), w_off), "offsets differ from the reference"
    assert np.array_equal(d_out[:T].cpu().numpy(), w_flat), "text differs from the reference"
    ms = (ctypes.c_float * 6)()
    L.BfLastKernelMs(VP(h), ms, 6)
    segments = dict(zip(("prep", "walk", "scan", "copy", "total", "walk_kernel"), [round(float(x), 4) for x in ms]))
    if a.once:
        print(json.dumps({"words": n, "verified": True, "kernel_ms": segments}))
        bf.free_model(h)
        return

    gpu = []
    for _ in range(a.windows):
        reps, elapsed = 0, 0.0
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        while True:
            for _ in range(8):
                call()
            reps += 8
            e1.record(stream)
            e1.synchronize()
            elapsed = e0.elapsed_time(e1) / 1e3
            if elapsed >= 1.0:
                break
        gpu.append(n * reps / elapsed)
    bf.free_model(h)

    cpu = []
    if not a.no_cpu and bfutil.have_ref():
        D = ctypes.CDLL(os.path.join(ROOT, "tools", "libw2hcpu.so"))
        D.w2h_cpu_pass.restype = ctypes.c_double
        D.w2h_cpu_pass.argtypes = [VP, VP, ctypes.c_int64, ctypes.c_int, ctypes.c_int, VP, VP]
        D.w2h_cpu_open.argtypes = [ctypes.c_char_p, ctypes.c_char_p]
        assert D.w2h_cpu_open(bfutil.REF_LIB.encode(), wc.FIXTURE.encode()) == 0
        nb, nf = ctypes.c_int64(0), ctypes.c_int64(0)
        for k in range(a.windows + 1):
            passes, elapsed = 0, 0.0
            while elapsed < 1.0:                                # a window: whole passes over the same words until it is at least one second
                t = D.w2h_cpu_pass(flat.ctypes.data, off.ctypes.data, n, a.threads, 0x2D, ctypes.byref(nb), ctypes.byref(nf))
                assert t > 0 and nb.value == T and nf.value == 0, (t, nb.value, T, nf.value)
                passes, elapsed = passes + 1, elapsed + t
            if k:                                               # (the first window warms the caches)
                cpu.append(n * passes / elapsed)
        D.w2h_cpu_close()

    def summary(v):
        return {"median_words_per_s": statistics.median(v), "min": min(v), "max": max(v), "windows": len(v)} if v else None
    res = {"words": n, "input_bytes": total, "output_bytes": T, "verified": True, "device": torch.cuda.get_device_name(0), "kernel_ms_one_call": segments,
           "gpu_device_resident": summary(gpu), "reference_cpu": summary(cpu), "reference_threads": a.threads, "cpu": bfutil.cpu_model_string()}
    if gpu and cpu:
        res["speedup_of_medians"] = statistics.median(gpu) / statistics.median(cpu)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
