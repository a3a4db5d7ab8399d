"""MEASUREMENT: the offset conversions (ByteToCharOffsetsBatchDevice / CharToByteOffsetsBatchDevice) on text that is resident in HBM, beside a plain
copy of the text and beside the tokenizer step they follow, in one process.

Two workloads: config2 (English, bert_base_tok.bin) and config4 (multilingual, xlm_roberta_base.bin) of tests/bfutil.py.  The text is tokenised
once with offsets on the device (TextToIdsWithOffsetsBatchDevice); the items are its ragged starts / ends with its id offsets.  Every entry of
every output (both units, both directions) is verified first against the array form of the restatement of tests/charpos_cases.py, which the CPU
tests hold to the loop of the definition.

Timed, UTF-16 units (both masks), ends exclusive:

  index / scan / items   the three stages of one ByteToCharOffsetsBatchDevice call from the events BfLastKernelMs reads ([0] k_char_index, [2] the
                         scan of the chunk counts, [3] k_char_docs + k_char_fwd), median of `--calls` calls; `inv_items` the same of the inverse call
                         (k_char_docs + k_char_inv) over the converted offsets
  fwd_call / inv_call    a whole call, in windows of at least `--window-seconds` (device events around a window, calls back to back on one stream)
  copy                   one hipMemcpyAsync, device to device, of total_bytes -- the yardstick of the index pass, which reads the text once
  tokenizer              the TextToIdsWithOffsetsBatchDevice step the conversion follows
  encode_byte / _char    encode_batch_device(..., return_offsets=True) with offset_unit="byte" and "char" (rows of 128 cells, one row a document)
  large                  both texts above fit in the 256 MB last-level cache; config 4's text `--repeat` times end to end (2 GB by default) does not:
                         the index pass alone (the document units are its only output, verified by their repetition) beside the copy of that text

Writes profiles/charpos_bench.json.

  python tools/bench_charpos.py [--docs 200000] [--windows 5] [--calls 21] [--out profiles/charpos_bench.json]"""
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
    ap.add_argument("--docs", type=int, default=200000)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--calls", type=int, default=21)
    ap.add_argument("--repeat", type=int, default=20, help="config 4's text this many times end to end for the run beyond the last-level cache (1 = skip it)")
    ap.add_argument("--window-seconds", type=float, default=0.5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "charpos_bench.json"))
    a = ap.parse_args()

    import torch
    import bfutil
    import blingfire_amd as bf
    import charpos_cases as cc

    if not torch.cuda.is_available():
        sys.exit("bench_charpos.py measures on the GPU: no device is visible")
    VP = ctypes.c_void_p
    lib = bf.lib()
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream()
    sp = VP(stream.cuda_stream)
    hip = ctypes.CDLL("libamdhip64.so")                         # the HIP runtime torch and the library already run on
    hip.hipMemcpyAsync.restype = ctypes.c_int
    hip.hipMemcpyAsync.argtypes = [VP, VP, ctypes.c_size_t, ctypes.c_int, VP]
    p = lambda t: t.data_ptr()                                                               # noqa: E731

    def summary(v):
        return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "n": len(v)}

    def window(fn):
        reps = 0
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        while True:
            for _ in range(4):
                fn()
            reps += 4
            e1.record(stream)
            e1.synchronize()
            ms = e0.elapsed_time(e1)
            if ms >= a.window_seconds * 1e3:
                return ms / reps

    res = {"docs": a.docs, "unit_timed": "utf16", "verified": True, "device": torch.cuda.get_device_name(0), "window_seconds": a.window_seconds, "workloads": {}}
    for name in ("config2", "config4"):
        wl = bfutil.WORKLOADS[name]
        model = wl["model"] or "bert_base_tok.bin"
        text, off = bfutil.gen_corpus_multi(a.docs, **wl["multi"]) if "multi" in wl else bfutil.gen_corpus(a.docs, **wl["gen"])
        total, ndocs = int(off[-1]), len(off) - 1
        h = bf.load_model(bfutil.model_path(model))
        d_text, d_off = torch.from_numpy(text).to(dev), torch.from_numpy(off).to(dev)
        assert lib.BfReserve(VP(h), ndocs, total, 1) == 0
        tok = lambda: bf.text_to_ids_with_offsets_batch_device(h, d_text, d_off, wl["max_ids"], wl["unk"])      # noqa: E731
        d_ids, d_st, d_en, d_idoff = tok()
        torch.cuda.synchronize()
        assert lib.BfLastStatus(VP(h)) == 0
        n = int(d_idoff[-1].item())
        o_s, o_e = torch.empty_like(d_st), torch.empty_like(d_en)
        b_s, b_e = torch.empty_like(d_st), torch.empty_like(d_en)
        d_units = torch.empty(ndocs, dtype=torch.int32, device=dev)

        def fwd(unit=1, flags=2):
            r = lib.ByteToCharOffsetsBatchDevice(VP(h), p(d_text), p(d_off), ndocs, total, p(d_idoff), n, p(d_st), p(d_en), unit, flags, p(o_s), p(o_e), p(d_units), sp)
            assert r == 0, r

        def inv(unit=1, flags=3):
            r = lib.CharToByteOffsetsBatchDevice(VP(h), p(d_text), p(d_off), ndocs, total, p(d_idoff), n, p(o_s), p(o_e), unit, flags, p(b_s), p(b_e), None, sp)
            assert r == 0, r

        # ---- verification: every entry, both units; the inverse call takes the forward call's answers back to the bytes
        st_h, en_h, idoff_h = d_st.cpu().numpy()[:n], d_en.cpu().numpy()[:n], d_idoff.cpu().numpy()
        for unit in (0, 1):
            fwd(unit)
            inv(unit)
            torch.cuda.synchronize()
            assert lib.BfLastStatus(VP(h)) == 0
            ws, we, wu, wst = cc.restate_array(text, off, unit, cc.FWD, 2, st_h, en_h, idoff_h)
            assert wst == 0 and np.array_equal(o_s.cpu().numpy()[:n], ws) and np.array_equal(o_e.cpu().numpy()[:n], we) and np.array_equal(d_units.cpu().numpy(), wu), name
            bs, be, _, bst = cc.restate_array(text, off, unit, cc.INV, 3, ws, we, idoff_h)
            assert bst == 0 and np.array_equal(b_s.cpu().numpy()[:n], bs) and np.array_equal(b_e.cpu().numpy()[:n], be), name
            assert np.array_equal(bs, np.where(st_h >= 0, st_h, -1)) and np.array_equal(be[en_h >= 0], en_h[en_h >= 0] + 1), name      # and back where they came from
        print("%s: %d documents, %d bytes, %d tokens: verified" % (name, ndocs, total, n), file=sys.stderr, flush=True)
        multibyte = float(((text & 0xC0) == 0x80).mean())
        del st_h, en_h

        d_src, d_dst = d_text, torch.empty_like(d_text)

        def copy():
            r = hip.hipMemcpyAsync(p(d_dst), p(d_src), total, 3, sp)                         # 3 = hipMemcpyDeviceToDevice
            assert r == 0, r

        def stages(fn):
            ms = (ctypes.c_float * 6)()
            rows = []
            for _ in range(a.calls):
                fn()
                assert lib.BfLastKernelMs(VP(h), ms, 6) >= 5
                rows.append((ms[0], ms[2], ms[3], ms[4]))
            return [summary([r[k] for r in rows]) for k in range(4)]
        fwd(); inv(); copy()
        torch.cuda.synchronize()
        f_index, f_scan, f_items, f_total = stages(fwd)
        _, _, i_items, _ = stages(inv)
        L = 128
        enc = lambda unit: (lambda: bf.encode_batch_device(h, d_text, d_off, L, 0, 2, 1, wl["unk"], return_offsets=True, offset_unit=unit))      # noqa: E731
        fns = [("fwd_call", fwd), ("inv_call", inv), ("copy", copy), ("tokenizer", tok), ("encode_byte", enc("byte")), ("encode_char", enc("char"))]
        for _, fn in fns:
            fn()
        torch.cuda.synchronize()
        times = {k: [] for k, _ in fns}
        for _ in range(a.windows):
            for k, fn in fns:
                times[k].append(window(fn))
        out = {"model": model, "docs": ndocs, "text_bytes": total, "tokens": n, "continuation_byte_share": multibyte, "chunks": (total + 63) // 64,
               "index": f_index, "scan": f_scan, "items_fwd": f_items, "items_inv": i_items, "fwd_events_total": f_total}
        for k in times:
            out[k] = summary(times[k])
        med = {k: statistics.median(v) for k, v in times.items()}
        out.update({"index_over_copy": f_index["median_ms"] / med["copy"], "index_gb_per_s": total / f_index["median_ms"] / 1e6, "copy_gb_per_s_read": total / med["copy"] / 1e6,
                    "fwd_call_over_tokenizer": med["fwd_call"] / med["tokenizer"], "encode_char_over_byte": med["encode_char"] / med["encode_byte"]})
        # ---- beyond the last-level cache: the same text `--repeat` times end to end (the documents with it), the index pass alone
        # (d_doc_units_out is the only output: no items), verified by the document units, which repeat with the text
        if name == "config4" and a.repeat > 1:
            k = a.repeat
            big_text = d_text.repeat(k)
            big_off = torch.cat([d_off[:-1] + i * total for i in range(k)] + [torch.tensor([k * total], dtype=torch.int64, device=dev)])
            big_dst = torch.empty_like(big_text)
            big_units = torch.empty(k * ndocs, dtype=torch.int32, device=dev)

            def big_index():
                r = lib.ByteToCharOffsetsBatchDevice(VP(h), p(big_text), p(big_off), k * ndocs, k * total, None, 0, None, None, 1, 0, None, None, p(big_units), sp)
                assert r == 0, r

            def big_copy():
                r = hip.hipMemcpyAsync(p(big_dst), p(big_text), k * total, 3, sp)
                assert r == 0, r
            big_index(); big_copy()
            torch.cuda.synchronize()
            assert lib.BfLastStatus(VP(h)) == 0 and torch.equal(big_units, d_units.repeat(k)), "the large text's document units differ"
            b_index, b_scan, b_docs, _ = stages(big_index)
            b_copy = [window(big_copy) for _ in range(a.windows)]
            out["large"] = {"repeat": k, "text_bytes": k * total, "docs": k * ndocs, "index": b_index, "scan": b_scan, "docs_kernel": b_docs, "copy": summary(b_copy),
                            "index_over_copy": b_index["median_ms"] / statistics.median(b_copy), "index_gb_per_s": k * total / b_index["median_ms"] / 1e6,
                            "copy_gb_per_s_read": k * total / statistics.median(b_copy) / 1e6}
            del big_text, big_off, big_dst, big_units
        res["workloads"][name] = out
        bf.free_model(h)
        del d_text, d_off, d_ids, d_st, d_en, d_idoff, o_s, o_e, b_s, b_e, d_dst, d_src
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
