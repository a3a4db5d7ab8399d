"""MEASUREMENT: the companion planes of the row stage (k_rowstage_planes) and the span cells (k_rows_span) beside plain copies of their bytes,
beside the fill at the same shape, and the base calls beside the same calls of another build of the library.

1 M + 1 documents of bfutil.gen_corpus (workload config2) under bert_base_tok.bin are tokenised once on the device with offsets (max_len = 125);
the two companion arrays are the tokenizer's starts and ends, fill -1.  Rows: sequence q = document q at L = 64; pairs: A = document q,
B = document q + 1 at L = 128, mode 0 with max_a = 32, offsets over B alone; one row per item, [CLS] / [SEP] set.  Every output of every timed
call is verified first: the base outputs against the array forms of the restatements (tests/rows_cases.py, tests/pair_cases.py), the planes
against tests/plane_cases.py, the span cells against an array form of the definition that is itself held to plane_cases.restate_span on a
sample of the rows.

Timed in this process in alternating windows of at least one second each (device events around a window, calls back to back on one stream, a
warm-up call of each before the first window), median of `--windows` windows with the spread:

  rows_map          IdsToRowsBatchDevice, a row's item alone: count, scan, map -- what every call below starts with
  rows_fill         IdsToRowsBatchDevice, ids and mask alone: + k_rowstage_fill
  rows_planes       IdsToRowsPlanesBatchDevice, two planes alone: + k_rowstage_planes
  planes_copy       one hipMemcpyAsync, device to device, of the bytes k_rowstage_planes writes (two planes)
  rows_base         IdsToRowsBatchDevice, every output (the call as its users make it); with --parent-lib also through that library
  rows_all          IdsToRowsPlanesBatchDevice, every output and two planes
  pairs_base, pairs_all, pairs_map, pairs_fill, pairs_planes, pairs_planes_copy   the same for pairs at L = 128
  span              RowsSpanCellsBatchDevice over the two row planes (L = 64), one answer per document
  span_copy         one hipMemcpyAsync of the two planes it reads

A kernel's own time is reported BY DIFFERENCE of two calls that differ in that kernel alone (rows_planes - rows_map, rows_fill - rows_map); it is
named so in the result.  Writes profiles/planes_bench.json.

  python tools/bench_planes.py [--docs 1000000] [--windows 5] [--parent-lib other/libblingfiretokdll.so] [--out profiles/planes_bench.json]"""
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


def span_array_form(S, E, a, z, none):
    """the definition of RowsSpanCellsBatchDevice for row r = item r, as array operations"""
    L = S.shape[1]
    ok = S >= 0
    lo = ok & (S <= a[:, None]); hi = ok & (E >= z[:, None])
    found = (a >= 0) & (z >= a) & lo.any(axis=1) & hi.any(axis=1)
    start = np.where(found, L - 1 - np.argmax(lo[:, ::-1], axis=1), none).astype(np.int32)
    end = np.where(found, np.argmax(hi, axis=1), none).astype(np.int32)
    return start, end


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1000000)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--window-seconds", type=float, default=1.0)
    ap.add_argument("--parent-lib", default=None, help="another build of libblingfiretokdll.so: its base calls are timed in the same windows")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "planes_bench.json"))
    a = ap.parse_args()

    import torch
    import bfutil
    import blingfire_amd as bf
    import pair_cases as pc
    import plane_cases as pl
    import rows_cases as rc

    if not torch.cuda.is_available():
        sys.exit("bench_planes.py measures on the GPU: no device is visible")
    VP, I32 = ctypes.c_void_p, ctypes.c_int32
    LR, LP, CLS, SEP, PAD, UNK, MAX_A = 64, 128, 101, 102, 0, 100, 32
    wl = bfutil.WORKLOADS["config2"]
    n = a.docs
    text, off = bfutil.gen_corpus(n + 1, **wl["gen"])
    total = int(off[-1])
    lib = bf.lib()
    model = bfutil.model_path("bert_base_tok.bin")
    h = bf.load_model(model)
    dev = torch.device("cuda:0")
    d_text, d_off = torch.from_numpy(text).to(dev), torch.from_numpy(off).to(dev)
    max_len = LP - 3
    ids_cap = (n + 1) * max_len
    d_ids, d_st, d_en = (torch.empty(ids_cap, dtype=torch.int32, device=dev) for _ in range(3))
    d_idoff = torch.empty(n + 2, dtype=torch.int64, device=dev)
    d_offa, d_offb = d_idoff[:n + 1], d_idoff[1:]
    d_rows = torch.empty((n, LP), dtype=torch.int32, device=dev)
    d_mask = torch.empty((n, LP), dtype=torch.uint8, device=dev)
    d_type = torch.empty((n, LP), dtype=torch.uint8, device=dev)
    d_seq = torch.empty(n, dtype=torch.int32, device=dev)
    d_first = torch.empty(n, dtype=torch.int32, device=dev)
    d_roff = torch.empty(n + 1, dtype=torch.int64, device=dev)
    d_pl = [torch.empty((n, LP), dtype=torch.int32, device=dev) for _ in range(2)]          # (the rows form uses the first n * LR cells of each)
    d_cells = [torch.empty(n, dtype=torch.int32, device=dev) for _ in range(2)]
    d_src = torch.zeros(2 * n * LP * 4, dtype=torch.uint8, device=dev)
    d_dst = torch.empty(2 * n * LP * 4, dtype=torch.uint8, device=dev)
    assert lib.BfReserve(VP(h), n + 1, total, 1) == 0
    stream = torch.cuda.current_stream()
    sp = VP(stream.cuda_stream)
    hip = ctypes.CDLL("libamdhip64.so")                         # the HIP runtime torch and the library already run on
    hip.hipMemcpyAsync.restype = ctypes.c_int
    hip.hipMemcpyAsync.argtypes = [VP, VP, ctypes.c_size_t, ctypes.c_int, VP]

    r = lib.TextToIdsWithOffsetsBatchDevice(VP(h), d_text.data_ptr(), d_off.data_ptr(), n + 1, total, d_ids.data_ptr(), d_st.data_ptr(), d_en.data_ptr(), ids_cap,
                                            d_idoff.data_ptr(), max_len, UNK, sp)
    assert r == 0, r
    torch.cuda.synchronize()
    assert lib.BfLastStatus(VP(h)) == 0

    c_src = (VP * 2)(d_st.data_ptr(), d_en.data_ptr())
    c_fill = (I32 * 2)(-1, -1)
    c_out = (VP * 2)(d_pl[0].data_ptr(), d_pl[1].data_ptr())
    p = lambda t: t.data_ptr()                                                               # noqa: E731

    def rows_call(L_, handle, outs, planes):
        pre = (VP(handle), p(d_ids), ids_cap, p(d_offa), n, LR, CLS, SEP, PAD, 0, 1, 0, *outs, n, p(d_roff))
        r = L_.IdsToRowsPlanesBatchDevice(*pre, 2, c_src, c_fill, c_out, sp) if planes else L_.IdsToRowsBatchDevice(*pre, sp)
        assert r == 0, r

    def pairs_call(L_, handle, outs, planes):
        pre = (VP(handle), p(d_ids), ids_cap, p(d_offa), p(d_ids), ids_cap, p(d_offb), n, LP, CLS, SEP, PAD, 0, MAX_A, 0, 1, 0, *outs, n, p(d_roff))
        r = L_.IdsToPairRowsPlanesBatchDevice(*pre, 2, None, c_src, c_fill, c_out, sp) if planes else L_.IdsToPairRowsBatchDevice(*pre, sp)
        assert r == 0, r

    R_ALL, R_MAP, R_FILL, R_NONE = (p(d_rows), p(d_mask), p(d_seq), p(d_first)), (None, None, p(d_seq), None), (p(d_rows), p(d_mask), None, None), (None,) * 4
    P_ALL, P_MAP, P_FILL, P_NONE = (p(d_rows), p(d_mask), p(d_type), p(d_seq), p(d_first)), (None, None, None, p(d_seq), None), (p(d_rows), p(d_mask), p(d_type), None, None), (None,) * 5
    rows_bytes, pairs_bytes = 2 * n * LR * 4, 2 * n * LP * 4

    # answers: tokens 5 .. 7 of every document that has them
    ids_h, st_h, en_h, idoff_h = d_ids.cpu().numpy(), d_st.cpu().numpy(), d_en.cpu().numpy(), d_idoff.cpu().numpy()
    nid = int(idoff_h[-1])
    ids_h, st_h, en_h = ids_h[:nid], st_h[:nid], en_h[:nid]
    lens = np.diff(idoff_h[:n + 1])
    has = lens > 7
    ans_a = np.where(has, st_h[np.minimum(idoff_h[:n] + 5, nid - 1)], -1).astype(np.int32)
    ans_z = np.where(has, en_h[np.minimum(idoff_h[:n] + 7, nid - 1)], -1).astype(np.int32)
    d_a, d_z = torch.from_numpy(ans_a).to(dev), torch.from_numpy(ans_z).to(dev)

    def span():
        r = lib.RowsSpanCellsBatchDevice(VP(h), p(d_pl[0]), p(d_pl[1]), LR, n, d_roff.data_ptr() + 8 * n, None, n, p(d_a), p(d_z), 0, p(d_cells[0]), p(d_cells[1]), sp)
        assert r == 0, r

    def copy(nbytes):
        r = hip.hipMemcpyAsync(d_dst.data_ptr(), d_src.data_ptr(), nbytes, 3, sp)           # 3 = hipMemcpyDeviceToDevice
        assert r == 0, r

    # ---- verification of every timed call's outputs
    def same(what, got, want):
        assert np.array_equal(got, want), "%s differ from the restatement" % what
    want_rows = rc.restate_truncated(ids_h, idoff_h[:n + 1], LR, CLS, SEP, PAD)
    want_rpl = pl.restate_planes_truncated(idoff_h[:n + 1], LR, [st_h, en_h], [-1, -1])[0]
    rows_call(lib, h, R_ALL, True)
    torch.cuda.synchronize()
    assert lib.BfLastStatus(VP(h)) == 0
    for what, got, w in zip(("rows", "mask", "row_seq", "row_first", "row_offsets"), (d_rows.view(-1)[:n * LR], d_mask.view(-1)[:n * LR], d_seq, d_first, d_roff), want_rows):
        same("rows_all: " + what, got.cpu().numpy(), w.reshape(-1))
    S, E = (t.view(-1)[:n * LR].cpu().numpy().reshape(n, LR) for t in d_pl)
    same("rows_all: starts plane", S, want_rpl[0]); same("rows_all: ends plane", E, want_rpl[1])
    span()
    torch.cuda.synchronize()
    assert lib.BfLastStatus(VP(h)) == 0
    want_cells = span_array_form(S, E, ans_a, ans_z, 0)
    pick = np.concatenate([np.arange(1000), np.random.RandomState(1).randint(0, n, size=1000)]) if n > 2000 else np.arange(n)
    sample = pl.restate_span(S[pick], E[pick], None, len(pick), ans_a[pick], ans_z[pick], 0)
    same("the array form of the span definition (start)", want_cells[0][pick], sample[0]); same("the array form of the span definition (end)", want_cells[1][pick], sample[1])
    same("span: start cells", d_cells[0].cpu().numpy(), want_cells[0]); same("span: end cells", d_cells[1].cpu().numpy(), want_cells[1])
    found = float((want_cells[0] != want_cells[1]).mean())
    for t in d_pl:
        t.fill_(-7)
    rows_call(lib, h, R_NONE, True)                                                          # the planes alone
    torch.cuda.synchronize()
    same("rows_planes: starts plane", d_pl[0].view(-1)[:n * LR].cpu().numpy().reshape(n, LR), want_rpl[0])
    same("rows_planes: ends plane", d_pl[1].view(-1)[:n * LR].cpu().numpy().reshape(n, LR), want_rpl[1])
    rows_call(lib, h, R_ALL, False)
    torch.cuda.synchronize()
    for what, got, w in zip(("rows", "mask", "row_seq", "row_first", "row_offsets"), (d_rows.view(-1)[:n * LR], d_mask.view(-1)[:n * LR], d_seq, d_first, d_roff), want_rows):
        same("rows_base: " + what, got.cpu().numpy(), w.reshape(-1))
    del want_rows, want_rpl, S, E
    want_pairs = pc.restate_one_row(ids_h, idoff_h[:-1], ids_h, idoff_h[1:], LP, CLS, SEP, PAD, 0, MAX_A)
    cells = pc.restate_one_row(pl._index_ids(nid, pl.BASE_A), idoff_h[:-1], pl._index_ids(nid, pl.BASE_B), idoff_h[1:], LP, CLS, SEP, pl.PAD_MARK, 0, MAX_A)[0]
    want_ppl = [pl._gather(cells, pl.BASE_B, 1 << 31, s, -1) for s in (st_h, en_h)]
    del cells
    for planes in (True, False):
        pairs_call(lib, h, P_ALL, planes)
        torch.cuda.synchronize()
        assert lib.BfLastStatus(VP(h)) == 0
        for what, got, w in zip(("rows", "mask", "type", "row_seq", "row_first_b", "row_offsets"), (d_rows, d_mask, d_type, d_seq, d_first, d_roff), want_pairs):
            same("pairs %s: %s" % ("all" if planes else "base", what), got.cpu().numpy(), w)
        if planes:
            same("pairs_all: starts plane", d_pl[0].cpu().numpy(), want_ppl[0]); same("pairs_all: ends plane", d_pl[1].cpu().numpy(), want_ppl[1])
            for t in d_pl:
                t.fill_(-7)
            pairs_call(lib, h, P_NONE, True)
            torch.cuda.synchronize()
            same("pairs_planes: starts plane", d_pl[0].cpu().numpy(), want_ppl[0]); same("pairs_planes: ends plane", d_pl[1].cpu().numpy(), want_ppl[1])
    del want_ppl

    fns = [("rows_map", lambda: rows_call(lib, h, R_MAP, False)), ("rows_fill", lambda: rows_call(lib, h, R_FILL, False)),
           ("rows_planes", lambda: rows_call(lib, h, R_NONE, True)), ("planes_copy", lambda: copy(rows_bytes)),
           ("rows_base", lambda: rows_call(lib, h, R_ALL, False)), ("rows_all", lambda: rows_call(lib, h, R_ALL, True)),
           ("pairs_map", lambda: pairs_call(lib, h, P_MAP, False)), ("pairs_fill", lambda: pairs_call(lib, h, P_FILL, False)),
           ("pairs_planes", lambda: pairs_call(lib, h, P_NONE, True)), ("pairs_planes_copy", lambda: copy(pairs_bytes)),
           ("pairs_base", lambda: pairs_call(lib, h, P_ALL, False)), ("pairs_all", lambda: pairs_call(lib, h, P_ALL, True))]
    hp = None
    if a.parent_lib:
        plib = ctypes.CDLL(os.path.abspath(a.parent_lib))
        plib.LoadModel.restype = VP; plib.LoadModel.argtypes = [ctypes.c_char_p]
        plib.FreeModel.argtypes = [VP]
        plib.BfReserve.argtypes = [VP, ctypes.c_int64, ctypes.c_int64, ctypes.c_int]
        plib.IdsToRowsBatchDevice.argtypes = lib.IdsToRowsBatchDevice.argtypes
        plib.IdsToPairRowsBatchDevice.argtypes = lib.IdsToPairRowsBatchDevice.argtypes
        hp = plib.LoadModel(model.encode("utf-8"))
        assert hp and plib.BfReserve(VP(hp), n + 1, total, 0) == 0
        for name, call, outs, L_ in (("rows_base", rows_call, R_ALL, LR), ("pairs_base", pairs_call, P_ALL, LP)):          # the other build computes the same
            got = []
            for which, handle in ((lib, h), (plib, hp)):
                for t in (d_rows, d_mask, d_type, d_seq, d_first, d_roff):
                    t.fill_(0)
                call(which, handle, outs, False)
                torch.cuda.synchronize()
                got.append([t.clone() for t in (d_rows, d_mask, d_type, d_seq, d_first, d_roff)])
            assert all(torch.equal(x, y) for x, y in zip(*got)), "%s: the two builds differ" % name
            del got
        fns += [("parent_rows_base", lambda: rows_call(plib, hp, R_ALL, False)), ("parent_pairs_base", lambda: pairs_call(plib, hp, P_ALL, False))]
    del want_pairs
    rows_call(lib, h, R_ALL, True)                                                           # the planes the span call reads
    fns += [("span", span), ("span_copy", lambda: copy(rows_bytes))]
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
    if hp:
        plib.FreeModel(VP(hp))

    def summary(v):
        return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "windows": len(v)}
    med = {k: statistics.median(v) for k, v in times.items()}
    res = {"docs": n, "text_bytes": total, "ids": nid, "model": "bert_base_tok.bin", "workload": "config2", "rows_row_len": LR, "pairs_row_len": LP, "max_len": max_len,
           "pairs_max_a": MAX_A, "planes": 2, "verified": True, "answers_found_share": found, "device": torch.cuda.get_device_name(0), "window_seconds": a.window_seconds}
    for name in times:
        res[name] = summary(times[name])
    k_rp, k_rf = med["rows_planes"] - med["rows_map"], med["rows_fill"] - med["rows_map"]
    k_pp, k_pf = med["pairs_planes"] - med["pairs_map"], med["pairs_fill"] - med["pairs_map"]
    res.update({"rows_planes_bytes_written": rows_bytes, "pairs_planes_bytes_written": pairs_bytes, "span_bytes_read": rows_bytes,
                "by_difference_ms": {"k_rowstage_planes_rows": k_rp, "k_rowstage_fill_rows": k_rf, "k_rowstage_planes_pairs": k_pp, "k_rowstage_fill_pairs": k_pf},
                "k_rowstage_planes_rows_over_copy": k_rp / med["planes_copy"], "k_rowstage_planes_rows_over_fill": k_rp / k_rf,
                "k_rowstage_planes_pairs_over_copy": k_pp / med["pairs_planes_copy"], "k_rowstage_planes_pairs_over_fill": k_pp / k_pf,
                "k_rowstage_planes_rows_written_GBps": rows_bytes / k_rp / 1e6, "k_rowstage_planes_pairs_written_GBps": pairs_bytes / k_pp / 1e6,
                "planes_copy_GBps": rows_bytes / med["planes_copy"] / 1e6, "pairs_planes_copy_GBps": pairs_bytes / med["pairs_planes_copy"] / 1e6,
                "span_over_span_copy": med["span"] / med["span_copy"], "span_read_GBps": rows_bytes / med["span"] / 1e6,
                "rows_all_over_rows_base": med["rows_all"] / med["rows_base"], "pairs_all_over_pairs_base": med["pairs_all"] / med["pairs_base"]})
    if a.parent_lib:
        res.update({"rows_base_over_parent": med["rows_base"] / med["parent_rows_base"], "pairs_base_over_parent": med["pairs_base"] / med["parent_pairs_base"]})
    else:
        res["parent"] = "not measured"
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
