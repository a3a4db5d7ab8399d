"""MEASUREMENT: the companion planes of the packed stage (k_packed_planes) beside a plain copy of the bytes they write, beside the fill of the same
call (k_packed_fill) and beside the companion planes of the rows stage (k_rowstage_planes) at the same L; and the base packed call beside the
same call of another build of the library.

1 M documents of bfutil.gen_corpus (workload config2) under bert_base_tok.bin are tokenised once on the device with offsets (max_len = the largest
L - 2); the two companion arrays are the tokenizer's starts and ends, fill -1; [CLS] / [SEP] set.  For L = 128 and L = 512 every output of every
timed call is verified first: one run of the sequential restatement (tests/packed_cases.py) over ids that are their own index gives the cells,
from which the rows and both planes follow as tests/packedplanes_cases.py has it; the planes of the rows stage against tests/plane_cases.py.

Timed in this process in alternating windows of at least one second each (device events around a window, calls back to back on one stream, a
warm-up call of each before the first window), median of `--windows` windows with the spread:

  chain         IdsToPackedRowsBatchDevice, the row starts alone: widths, scans, next, the doubling rounds, rows -- what every packed call below starts with
  fill          IdsToPackedRowsBatchDevice, rows, seg and pos alone: + k_packed_fill
  planes        IdsToPackedRowsPlanesBatchDevice, two planes alone: + k_packed_planes
  copy          one hipMemcpyAsync, device to device, of the bytes k_packed_planes writes (two planes of R rows)
  base          IdsToPackedRowsBatchDevice, every output (the call as its users make it); with --parent-lib also through that library
  all           IdsToPackedRowsPlanesBatchDevice, every output and two planes
  rows_map      IdsToRowsBatchDevice, a row's item alone, one row per document
  rows_planes   IdsToRowsPlanesBatchDevice, two planes alone: + k_rowstage_planes (n rows: more cells than the packed planes, so the rate is given too)

A kernel's own time is reported BY DIFFERENCE of two calls that differ in that kernel alone (planes - chain, fill - chain, rows_planes - rows_map),
and for the two packed kernels also from the events the call records (BfLastKernelMs slot 3, median of 21 synchronised calls).  Writes
profiles/packedplanes_bench.json.

  python tools/bench_packedplanes.py [--docs 1000000] [--windows 5] [--parent-lib other/libblingfiretokdll.so] [--out profiles/packedplanes_bench.json]"""
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
    ap.add_argument("--parent-lib", default=None, help="another build of libblingfiretokdll.so: its base packed call is timed in the same windows")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "packedplanes_bench.json"))
    a = ap.parse_args()

    import torch
    import bfutil
    import blingfire_amd as bf
    import packed_cases as pc
    import packedplanes_cases as pp
    import plane_cases as pl

    if not torch.cuda.is_available():
        sys.exit("bench_packedplanes.py measures on the GPU: no device is visible")
    VP, I32 = ctypes.c_void_p, ctypes.c_int32
    CLS, SEP, PAD, UNK = 101, 102, 0, 100
    wl = bfutil.WORKLOADS["config2"]
    n = a.docs
    text, off = bfutil.gen_corpus(n, **wl["gen"])
    total = int(off[-1])
    lib = bf.lib()
    model = bfutil.model_path("bert_base_tok.bin")
    h = bf.load_model(model)
    dev = torch.device("cuda:0")
    d_text, d_off = torch.from_numpy(text).to(dev), torch.from_numpy(off).to(dev)
    assert lib.BfReserve(VP(h), n, total, 1) == 0
    stream = torch.cuda.current_stream()
    sp = VP(stream.cuda_stream)
    hip = ctypes.CDLL("libamdhip64.so")                         # the HIP runtime torch and the library already run on
    hip.hipMemcpyAsync.restype = ctypes.c_int
    hip.hipMemcpyAsync.argtypes = [VP, VP, ctypes.c_size_t, ctypes.c_int, VP]

    max_len = max(a.row_lens) - 2
    ids_cap = min(total, n * max_len) + 1
    d_ids, d_st, d_en = (torch.empty(ids_cap, dtype=torch.int32, device=dev) for _ in range(3))
    d_idoff = torch.empty(n + 1, dtype=torch.int64, device=dev)
    r = lib.TextToIdsWithOffsetsBatchDevice(VP(h), d_text.data_ptr(), d_off.data_ptr(), n, total, d_ids.data_ptr(), d_st.data_ptr(), d_en.data_ptr(), ids_cap,
                                            d_idoff.data_ptr(), max_len, UNK, sp)
    assert r == 0, r
    torch.cuda.synchronize()
    assert lib.BfLastStatus(VP(h)) == 0
    idoff_h = d_idoff.cpu().numpy()
    nids = int(idoff_h[-1])
    ids_h, st_h, en_h = (t.cpu().numpy()[:nids] for t in (d_ids, d_st, d_en))
    del d_text
    c_src = (VP * 2)(d_st.data_ptr(), d_en.data_ptr())
    c_fill = (I32 * 2)(-1, -1)

    plib = hp = None
    if a.parent_lib:
        plib = ctypes.CDLL(os.path.abspath(a.parent_lib))
        plib.LoadModel.restype = VP; plib.LoadModel.argtypes = [ctypes.c_char_p]
        plib.FreeModel.argtypes = [VP]
        plib.BfReserve.argtypes = [VP, ctypes.c_int64, ctypes.c_int64, ctypes.c_int]
        plib.IdsToPackedRowsBatchDevice.argtypes = lib.IdsToPackedRowsBatchDevice.argtypes
        hp = plib.LoadModel(model.encode("utf-8"))
        assert hp and plib.BfReserve(VP(hp), n, total, 0) == 0

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

    res = {"docs": n, "text_bytes": total, "ids": nids, "model": "bert_base_tok.bin", "workload": "config2", "planes": 2, "verified": True,
           "device": torch.cuda.get_device_name(0), "window_seconds": a.window_seconds, "parent": "measured" if hp else "not measured", "row_lens": {}}
    p = lambda t: t.data_ptr()                                                               # noqa: E731
    for L in a.row_lens:
        d_nrows = torch.zeros(1, dtype=torch.int64, device=dev)
        pre = (d_ids.data_ptr(), ids_cap, d_idoff.data_ptr(), n, L, CLS, SEP, PAD, 0)
        assert lib.IdsToPackedRowsBatchDevice(VP(h), *pre, None, None, None, None, 0, None, None, p(d_nrows), sp) == 0      # the size query
        R = int(d_nrows.item())
        base_pl = [torch.empty((R, L), dtype=torch.int32, device=dev) for _ in range(3)]
        d_first = torch.empty(R + 1, dtype=torch.int32, device=dev)
        d_seq = [torch.empty(n, dtype=torch.int32, device=dev) for _ in range(2)]
        d_pl = [torch.empty((n, L), dtype=torch.int32, device=dev) for _ in range(2)]        # (the packed planes use the first R rows of each)
        c_out = (VP * 2)(p(d_pl[0]), p(d_pl[1]))
        r_seq = torch.empty(n, dtype=torch.int32, device=dev)
        r_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
        planes_bytes, rows_planes_bytes = 2 * R * L * 4, 2 * n * L * 4
        d_csrc = torch.zeros(planes_bytes, dtype=torch.uint8, device=dev)
        d_cdst = torch.empty(planes_bytes, dtype=torch.uint8, device=dev)
        O_ALL = (p(base_pl[0]), p(base_pl[1]), p(base_pl[2]), p(d_first), R, p(d_seq[0]), p(d_seq[1]))
        O_CHAIN = (None, None, None, p(d_first), R, None, None)
        O_FILL = (p(base_pl[0]), p(base_pl[1]), p(base_pl[2]), None, R, None, None)
        O_NONE = (None, None, None, None, R, None, None)

        def packed(L_, handle, outs, planes):
            if planes:
                r = L_.IdsToPackedRowsPlanesBatchDevice(VP(handle), *pre, *outs, p(d_nrows), 2, c_src, c_fill, c_out, sp)
            else:
                r = L_.IdsToPackedRowsBatchDevice(VP(handle), *pre, *outs, p(d_nrows), sp)
            assert r == 0, r

        def rows(planes):
            rpre = (VP(h), p(d_ids), ids_cap, p(d_idoff), n, L, CLS, SEP, PAD, 0, 1, 0, None, None, None if planes else p(r_seq), None, n, p(r_off))
            r = lib.IdsToRowsPlanesBatchDevice(*rpre, 2, c_src, c_fill, c_out, sp) if planes else lib.IdsToRowsBatchDevice(*rpre, sp)
            assert r == 0, r

        def copy():
            r = hip.hipMemcpyAsync(p(d_cdst), p(d_csrc), planes_bytes, 3, sp)                # 3 = hipMemcpyDeviceToDevice
            assert r == 0, r

        # ---- verification of every timed call's outputs
        def same(what, got, want):
            assert np.array_equal(got, want), "L %d: %s differ from the restatement" % (L, what)
        want = pc.restate(pp.BASE + np.arange(nids, dtype=np.int64), idoff_h, L, CLS, SEP, pp.PAD_MARK)
        assert want[6] == R, "the row count differs from the restatement"
        cells = want[0].astype(np.int64)
        holds = cells >= pp.BASE
        at = np.where(holds, cells - pp.BASE, 0)
        w_rows = np.where(holds, ids_h[at], np.where(cells == pp.PAD_MARK, PAD, cells)).astype(np.int32)
        w_pl = [np.where(holds, s[at], -1).astype(np.int32) for s in (st_h, en_h)]
        w_base = (w_rows,) + tuple(want[1:6])
        del want, cells, at
        names = ("rows", "seg", "pos", "row_first_seq", "seq_row", "seq_col")
        packed(lib, h, O_ALL, True)
        torch.cuda.synchronize()
        assert lib.BfLastStatus(VP(h)) == 0 and int(d_nrows.item()) == R
        for name, got, w in zip(names, (*base_pl, d_first, *d_seq), w_base):
            same("all: " + name, got.cpu().numpy(), w)
        for name, t, w in zip(("starts plane", "ends plane"), d_pl, w_pl):
            same("all: " + name, t.view(-1)[:R * L].cpu().numpy().reshape(R, L), w)
        for t in d_pl + base_pl + [d_first] + d_seq:
            t.fill_(-7)
        packed(lib, h, O_NONE, True)                                                        # the planes alone
        torch.cuda.synchronize()
        assert lib.BfLastStatus(VP(h)) == 0
        for name, t, w in zip(("starts plane", "ends plane"), d_pl, w_pl):
            same("planes: " + name, t.view(-1)[:R * L].cpu().numpy().reshape(R, L), w)
        handles = [(lib, h, "base")] + ([(plib, hp, "parent base")] if hp else [])
        for L_, handle, what in handles:
            for t in base_pl + [d_first] + d_seq:
                t.fill_(-7)
            packed(L_, handle, O_ALL, False)
            torch.cuda.synchronize()
            for name, got, w in zip(names, (*base_pl, d_first, *d_seq), w_base):
                same("%s: %s" % (what, name), got.cpu().numpy(), w)
        for outs, idx in ((O_FILL, (0, 1, 2)), (O_CHAIN, (3,))):
            for t in base_pl + [d_first]:
                t.fill_(-7)
            packed(lib, h, outs, False)
            torch.cuda.synchronize()
            for i in idx:
                same("partial: " + names[i], (*base_pl, d_first)[i].cpu().numpy(), w_base[i])
        real_cells = int(holds.sum())
        del w_base, w_rows, w_pl, holds
        w_rpl = pl.restate_planes_truncated(idoff_h, L, [st_h, en_h], [-1, -1])[0]
        rows(True)
        torch.cuda.synchronize()
        assert lib.BfLastStatus(VP(h)) == 0
        same("rows_planes: starts plane", d_pl[0].cpu().numpy(), w_rpl[0]); same("rows_planes: ends plane", d_pl[1].cpu().numpy(), w_rpl[1])
        del w_rpl
        print("L %d: %d rows, every output verified" % (L, R), file=sys.stderr, flush=True)

        # ---- the two packed kernels from the events of their calls
        def slot3(fn):
            buf, v = (ctypes.c_float * 6)(), []
            for _ in range(21):
                fn()
                assert lib.BfLastKernelMs(VP(h), buf, 6) == 6
                v.append(buf[3])
            return statistics.median(v)
        ev_fill = slot3(lambda: packed(lib, h, O_FILL, False))
        ev_planes = slot3(lambda: packed(lib, h, O_NONE, True))
        ev_both = slot3(lambda: packed(lib, h, O_ALL, True))

        fns = [("chain", lambda: packed(lib, h, O_CHAIN, False)), ("fill", lambda: packed(lib, h, O_FILL, False)), ("planes", lambda: packed(lib, h, O_NONE, True)),
               ("copy", copy), ("base", lambda: packed(lib, h, O_ALL, False)), ("all", lambda: packed(lib, h, O_ALL, True)),
               ("rows_map", lambda: rows(False)), ("rows_planes", lambda: rows(True))]
        if hp:
            fns.append(("parent_base", lambda: packed(plib, hp, O_ALL, False)))
        for _, fn in fns:
            fn()
        torch.cuda.synchronize()
        times = {name: [] for name, _ in fns}
        for _ in range(a.windows):
            for name, fn in fns:
                times[name].append(window(fn))
        med = {k: statistics.median(v) for k, v in times.items()}
        k_pl, k_fill, k_rpl = med["planes"] - med["chain"], med["fill"] - med["chain"], med["rows_planes"] - med["rows_map"]
        out = {"row_len": L, "packed_rows": R, "rows_stage_rows": n, "id_cell_share": real_cells / (R * L),
               "planes_bytes_written": planes_bytes, "fill_bytes_written": 3 * R * L * 4, "rows_planes_bytes_written": rows_planes_bytes}
        for name in times:
            out[name] = summary(times[name])
        out.update({"by_difference_ms": {"k_packed_planes": k_pl, "k_packed_fill": k_fill, "k_rowstage_planes": k_rpl},
                    "from_events_ms": {"k_packed_fill": ev_fill, "k_packed_planes": ev_planes, "k_packed_fill_and_planes": ev_both},
                    "k_packed_planes_over_copy": k_pl / med["copy"], "k_packed_planes_over_k_packed_fill": k_pl / k_fill,
                    "k_packed_planes_over_k_rowstage_planes": k_pl / k_rpl,
                    "k_packed_planes_written_GBps": planes_bytes / k_pl / 1e6, "k_packed_fill_written_GBps": 3 * R * L * 4 / k_fill / 1e6,
                    "k_rowstage_planes_written_GBps": rows_planes_bytes / k_rpl / 1e6, "copy_GBps": planes_bytes / med["copy"] / 1e6,
                    "all_over_base": med["all"] / med["base"]})
        if hp:
            out.update({"base_over_parent_base": med["base"] / med["parent_base"],
                        "base_median_within_parent_min_max": bool(min(times["parent_base"]) <= med["base"] <= max(times["parent_base"])),
                        "base_median_at_most_parent_max": bool(med["base"] <= max(times["parent_base"]))})
        res["row_lens"][str(L)] = out
        del base_pl, d_pl, d_csrc, d_cdst
        torch.cuda.empty_cache()
    bf.free_model(h)
    if hp:
        plib.FreeModel(VP(hp))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
