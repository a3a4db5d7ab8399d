"""CPU tier of the span-corruption call (RowsDenoiseBatchDevice): the lane code of blingfire_amd/csrc/bf_denoise.h (reach, segmented max-scan with its
chunk carry, begin test, run index and cap, running counts, the two positions), compiled for the host and driven in the kernel's partition
(tests/hosttest/bf_denoisetest.cpp), is held to the restatement of denoise_cases in all seven outputs and the status bit, on every case of the
table and every group size; the table is shown to contain what it is there for; the restatement's array form is held to its loop; the
invariants of the two rows; the refused arguments; denoise_start_prob; and the symbol is declared and exported."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import bfutil
import denoise_cases as dc
import mlm_cases as mc

c_i64, c_int, c_vp, c_dbl = ctypes.c_int64, ctypes.c_int, ctypes.c_void_p, ctypes.c_double
GROUPS = [1, 2, 4, 8, 16, 32, 64]


@pytest.fixture(scope="module")
def ht():
    L = ctypes.CDLL(bfutil.HOSTTEST_LIB)
    L.bft_denoise_rows.restype = c_int
    L.bft_denoise_rows.argtypes = [c_vp, c_int, c_i64, c_i64, c_vp, c_vp, c_int, c_vp, c_dbl] + [c_int] * 8 + [ctypes.c_uint64, ctypes.c_uint32] + [
        c_int, c_vp, c_vp, c_vp] * 2 + [c_vp, c_int, c_vp]
    L.bft_denoise_spec_ok.restype = c_int
    L.bft_denoise_spec_ok.argtypes = [c_int, c_vp, c_dbl] + [c_int] * 5
    return L


def host_denoise(ht, rows, mask=None, seg=None, row_base=0, enc_len=None, dec_len=None, group=0, **kw):
    """-> the seven outputs and the status word, as restate_denoise names them"""
    s = dc.spec_of(kw)
    rows = np.ascontiguousarray(rows, dtype=np.int32)
    R, L = rows.shape
    EL = L if enc_len is None else enc_len
    DL = L + 2 if dec_len is None else dec_len
    m = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
    g = None if seg is None else np.ascontiguousarray(seg, dtype=np.int32)
    out = {n: np.full((R, EL) if n.startswith("enc") and not n.endswith("count") else (R, DL) if n.startswith("dec") and not n.endswith("count") else (R,),
                      dc.CANARY32, dtype=np.int32) for n in dc.NAMES}
    sp = (ctypes.c_int32 * max(len(s["special_ids"]), 1))(*s["special_ids"])
    status = ctypes.c_int(-1)
    a = lambda x: None if x is None else x.ctypes.data
    r = ht.bft_denoise_rows(a(rows), L, R, row_base, a(m), a(g), len(s["special_ids"]), sp, s["start_prob"], s["len_lo"], s["len_hi"], s["sentinel_first"],
                            s["sentinel_step"], s["max_sentinels"], -1 if s["eos_id"] is None else s["eos_id"], s["pad_id"], s["ignore_label"], s["seed"], s["epoch"],
                            EL, a(out["enc"]), a(out["enc_cell"]), a(out["enc_count"]), DL, a(out["dec"]), a(out["dec_cell"]), a(out["dec_count"]), a(out["span_count"]),
                            group, ctypes.byref(status))
    assert r == 0
    out["status"] = status.value
    return out


def same(got, want, what=None):
    for name in dc.NAMES + ("status",):
        assert np.array_equal(got[name], want[name]), (name, what)
    return True


# ---- (a) the lane code against the restatement
@pytest.mark.parametrize("L", dc.HOST_L)
def test_a_every_group_size_equals_the_restatement(ht, L):
    for c, want in dc.table(L):
        for G in GROUPS + [0]:
            same(host_denoise(ht, c["rows"], c["mask"], c["seg"], group=G, **c["kw"]), want, (c["name"], G))


def test_a_row_indices_above_2_to_32(ht):
    rows, mask, seg = mc.random_rows(6, 65, 5)
    differ = []
    for base in (0, (1 << 32) + 3, (1 << 40) + 7):
        kw = dict(special_ids=dc.SPECIALS, start_prob=0.25, seed=9, row_base=base)
        want = dc.restate_denoise(rows, mask, seg, **kw)
        for G in (1, 64):
            same(host_denoise(ht, rows, mask, seg, group=G, **kw), want, (base, G))
        differ.append(want["dec"])
    assert not np.array_equal(differ[0], differ[1]) and not np.array_equal(differ[1], differ[2])          # the high word of the row index reaches the draw


def test_a_array_form_of_the_restatement_equals_the_loop():
    for L in dc.HOST_L:
        for c, want in dc.table(L):
            same(dc.restate_denoise(c["rows"], c["mask"], c["seg"], array=True, **c["kw"]), want, c["name"])


# ---- (b) the table holds what it is there for
def test_b_the_table_contains_its_claims():
    """read off the restatement's own output (denoise_cases.coverage); the GPU tier's lengths alone carry every claim too"""
    for Ls in (dc.HOST_L, dc.TABLE_L):
        found = dc.coverage(Ls)
        for claim in dc.CLAIMS:
            print("%3d  %s" % (len(found.get(claim, [])), claim))
            assert found.get(claim), (claim, len(Ls))


def test_b_start_prob_0_and_1(ht):
    for L in (9, 65, 129):
        c, w = dc.case_named(L, "none")
        for r in range(len(c["rows"])):                       # the encoder row is the present cells, the decoder row the eos alone
            assert w["enc"][r, :w["enc_count"][r]].tolist() == c["rows"][r][w["present"][r]].tolist()
            assert w["dec"][r].tolist() == [dc.EOS] + [-100] * (L + 1)
        c, w = dc.case_named(L, "all")
        for r, runs in enumerate(dc.runs_of(w["eligible"])):  # one run per stretch of eligible cells: one sentinel each in the encoder row
            assert w["span_count"][r] == len(runs) and w["enc_count"][r] == len(runs) + int((~w["eligible"][r]).sum())


# ---- (c) invariants
@pytest.mark.parametrize("L", dc.HOST_L)
def test_c_invariants(ht, L):
    for c, _ in dc.table(L):
        if "enc_len" in c["kw"]:
            continue                                          # (the truncated forms are prefixes: test_c_truncation)
        kw = dc.spec_of(c["kw"])
        got = host_denoise(ht, c["rows"], c["mask"], c["seg"], **c["kw"])
        present = mc.eligible(c["rows"], c["mask"], c["seg"], ())
        sentinels = {kw["sentinel_first"] + k * kw["sentinel_step"] for k in range(min(kw["max_sentinels"], L + 1))}
        assert (got["enc_count"] <= L).all() and (got["dec_count"] <= L + 2).all() and got["status"] == 0
        for r in range(len(c["rows"])):
            ne, nd, ns = int(got["enc_count"][r]), int(got["dec_count"][r]), int(got["span_count"][r])
            body = nd - (1 if kw["eos_id"] is not None else 0)
            enc, ecell, dec, dcell = got["enc"][r], got["enc_cell"][r], got["dec"][r], got["dec_cell"][r]
            assert (enc[ne:] == kw["pad_id"]).all() and (ecell[ne:] == -1).all() and (dec[nd:] == -100).all() and (dcell[nd:] == -1).all()
            if kw["eos_id"] is not None:
                assert dec[nd - 1] == kw["eos_id"] and dcell[nd - 1] == -1
            # the cell planes index the ids they sit beside; everything else is a sentinel, in run order on both sides
            for ids, cells, n in ((enc, ecell, ne), (dec, dcell, body)):
                at = cells[:n] >= 0
                assert np.array_equal(ids[:n][at], c["rows"][r][cells[:n][at]]) and (np.diff(cells[:n][at]) > 0).all()
                assert ids[:n][~at].tolist() == [kw["sentinel_first"] + k * kw["sentinel_step"] for k in range(ns)]
            # interleaved back: behind sentinel k of the encoder row go the ids behind sentinel k of the decoder row -> the present cells in order
            groups, k = {}, -1
            for i in range(body):
                if dcell[i] < 0:
                    k += 1
                    groups[k] = []
                else:
                    groups[k].append(int(dec[i]))
            back, k = [], 0
            for i in range(ne):
                if ecell[i] < 0:
                    back += groups[k]
                    k += 1
                else:
                    back.append(int(enc[i]))
            assert back == c["rows"][r][present[r]].tolist() and k == ns
            if not sentinels & set(c["rows"][r].tolist()):
                assert int(np.isin(enc[:ne], list(sentinels)).sum()) == ns


@pytest.mark.parametrize("L", [5, 33, 65, 129])
def test_c_truncation(ht, L):
    c, full = dc.case_named(L, "mixed")
    ne, nd = int(full["enc_count"].max()), int(full["dec_count"].max())
    for el, dl, status in ((ne, nd, 0), (ne - 1, nd, 1), (ne, nd - 1, 1), (ne - 1, nd - 1, 1)):
        if el < 1 or dl < 1:
            continue
        got = host_denoise(ht, c["rows"], c["mask"], c["seg"], enc_len=el, dec_len=dl, **c["kw"])
        assert got["status"] == status, (el, dl)
        assert np.array_equal(got["enc"], full["enc"][:, :el]) and np.array_equal(got["enc_cell"], full["enc_cell"][:, :el])
        assert np.array_equal(got["dec"], full["dec"][:, :dl]) and np.array_equal(got["dec_cell"], full["dec_cell"][:, :dl])
        assert np.array_equal(got["enc_count"], full["enc_count"]) and np.array_equal(got["dec_count"], full["dec_count"])          # the untruncated lengths


def test_c_a_second_epoch_and_a_second_seed_differ(ht):
    c, want = dc.case_named(129, "mixed")
    for change in (dict(epoch=c["kw"]["epoch"] + 1), dict(seed=c["kw"]["seed"] + 1)):
        other = host_denoise(ht, c["rows"], c["mask"], c["seg"], **dict(c["kw"], **change))
        assert not np.array_equal(other["enc"], want["enc"]) and not np.array_equal(other["dec"], want["dec"])
    same(host_denoise(ht, c["rows"], c["mask"], c["seg"], **c["kw"]), want)


def test_c_noise_density_of_the_default_spec():
    """8192 rows of 128 eligible cells at denoise_start_prob(0.15, 1, 5): an interior cell (four cells in front of it) is noise with probability 0.15.
    One cell's indicator has variance 0.1275; neighbours are correlated over at most 5 cells, so the mean over 1.0 M cells has a standard deviation
    below sqrt(0.1275 * 9 / 1.0e6) = 0.0011; asserted within 0.005"""
    import blingfire_amd as bf
    rows = np.full((8192, 128), 7, dtype=np.int32)
    w = dc.restate_denoise(rows, array=True, start_prob=bf.denoise_start_prob(0.15, 1, 5), len_lo=1, len_hi=5, seed=3, max_sentinels=1000, sentinel_first=30000,
                           sentinel_step=1)
    share = w["noise"][:, 4:].mean()
    print("noise share %.4f" % share)
    assert abs(share - 0.15) <= 0.005


# ---- (d) refused arguments
def test_d_denoise_spec_refuses_what_the_header_lists(ht):
    sp = (ctypes.c_int32 * 8)(1, 0, 102)
    nan = float("nan")

    def ok(nspecial=3, special=sp, prob=0.15, lo=1, hi=5, first=32099, step=-1, cap=100):
        return ht.bft_denoise_spec_ok(nspecial, special, prob, lo, hi, first, step, cap)
    good = [dict(), dict(nspecial=0, special=None), dict(nspecial=8), dict(prob=0.0), dict(prob=1.0), dict(lo=1 << 20, hi=1 << 20), dict(cap=1, first=0),
            dict(cap=1 << 20, first=0, step=1), dict(first=(1 << 31) - 1, step=-1), dict(first=99, step=-1, cap=100), dict(first=0, step=0),
            dict(first=(1 << 31) - 1 - 99, step=1, cap=100), dict(first=(1 << 31) - 1, step=-(1 << 31), cap=1)]
    for g in good:
        assert ok(**g) == 1, g
    bad = [dict(nspecial=-1), dict(nspecial=9), dict(nspecial=1, special=None), dict(prob=-0.01), dict(prob=1.01), dict(prob=nan), dict(lo=0), dict(lo=-1),
           dict(lo=6, hi=5), dict(hi=(1 << 20) + 1), dict(cap=0), dict(cap=-1), dict(cap=(1 << 20) + 1), dict(first=-1), dict(first=98, step=-1, cap=100),
           dict(first=(1 << 31) - 99, step=1, cap=100), dict(first=(1 << 31) - 1, step=(1 << 31) - 1, cap=3), dict(first=0, step=-(1 << 31), cap=2)]
    for b in bad:
        assert ok(**b) == 0, b


def test_d_the_call_refuses_what_the_header_lists(ht):
    """the driver checks what RowsDenoiseBatchDevice checks (all but the handle)"""
    rows = np.full((2, 8), 7, dtype=np.int32)
    outs = [np.zeros((2, 10), dtype=np.int32) for _ in range(4)] + [np.zeros(2, dtype=np.int32) for _ in range(3)]
    sp = (ctypes.c_int32 * 8)(1, 0, 102)

    def call(rows_=rows, row_len=8, n=2, enc_len=8, dec_len=10, take=(True,) * 7, prob=0.15, lo=1, hi=5, first=32099, step=-1, cap=100, nspecial=3, special=sp):
        o = [x.ctypes.data if t else None for x, t in zip(outs, take)]
        return ht.bft_denoise_rows(None if rows_ is None else rows_.ctypes.data, row_len, n, 0, None, None, nspecial, special, prob, lo, hi, first, step, cap, 1, 0, -100, 1, 0,
                                   enc_len, o[0], o[1], o[4], dec_len, o[2], o[3], o[5], o[6], 0, None)
    only = lambda i: tuple(j == i for j in range(7))
    counts = (False,) * 4 + (True,) * 3
    good = [dict(), dict(row_len=1, enc_len=1, dec_len=3), dict(n=0, rows_=None, take=(False,) * 7), dict(enc_len=0, dec_len=0, take=counts),
            dict(enc_len=-5, take=(False, False, True, True, True, True, True)), dict(dec_len=(1 << 20) + 1, take=(True, True, False, False, True, True, True)),
            dict(take=only(6)), dict(take=only(1)), dict(enc_len=1, dec_len=1)]
    for g in good:
        assert call(**g) == 0, g
    bad = [dict(row_len=0), dict(row_len=-1), dict(row_len=(1 << 20) + 1, n=0), dict(n=-1), dict(rows_=None), dict(take=(False,) * 7), dict(enc_len=0), dict(dec_len=0),
           dict(enc_len=(1 << 20) + 1), dict(dec_len=(1 << 20) + 1), dict(enc_len=0, take=only(1)), dict(dec_len=0, take=only(3)), dict(prob=float("nan")), dict(lo=0),
           dict(hi=0), dict(cap=0), dict(first=-1), dict(first=5, cap=7), dict(nspecial=9), dict(nspecial=1, special=None)]
    for b in bad:
        assert call(**b) == -1, b


# ---- (e) denoise_start_prob
def test_e_denoise_start_prob():
    import blingfire_amd as bf

    def density(p, lo, hi):
        clean = 1.0
        for k in range(hi):
            clean *= 1.0 - p * (1.0 if k < lo else (hi - k) / float(hi - lo + 1))
        return 1.0 - clean
    for lo, hi in ((1, 1), (1, 5), (3, 3), (2, 10), (1, 100)):
        last = -1.0
        for d in (0.0, 0.01, 0.05, 0.15, 0.3, 0.5, 0.9, 1.0):
            p = bf.denoise_start_prob(d, lo, hi)
            assert 0.0 <= p <= 1.0 and abs(density(p, lo, hi) - d) <= 1e-12, (d, lo, hi, p)
            assert p > last or (d == 0.0 and p == 0.0), (d, lo, hi)                  # monotone
            if (lo, hi) == (1, 1):
                assert abs(p - d) <= 1e-15                     # every span is its start: the density is the probability
            last = p
    assert 0.05 < bf.denoise_start_prob(0.15, 1, 5) < 0.06                          # (mean length 3: 3 p = 0.15 were there no overlaps; they cost a little)
    for bad in ((-0.1, 1, 5), (1.1, 1, 5), (float("nan"), 1, 5), (0.15, 0, 5), (0.15, 6, 5)):
        with pytest.raises(ValueError):
            bf.denoise_start_prob(*bad)


# ---- (f) declared and exported; the stand-alone program
def test_f_new_symbol_is_declared_and_exported():
    import blingfire_amd as bf
    hdr = open(os.path.join(bfutil.ROOT, "include", "blingfiretokdll_amd.h")).read()
    exports = open(os.path.join(bfutil.ROOT, "blingfire_amd", "csrc", "exports.map")).read()
    lib = ctypes.CDLL(bf.LIB_PATH)
    name = "RowsDenoiseBatchDevice"
    assert re.search(r"BF_API\s+\w+\s+%s\(" % name, hdr)
    assert re.search(r"^\s*%s;" % name, exports, flags=re.M)
    assert hasattr(lib, name)
    for fn in ("rows_denoise_device", "encode_denoise_batch_device", "denoise_start_prob"):
        assert callable(getattr(bf, fn))
    assert {"start_prob", "sentinel_first", "return_cells", "enc_len", "dec_len"} <= set(inspect.signature(bf.rows_denoise_device).parameters)
    assert "source" in inspect.signature(bf.encode_denoise_batch_device).parameters


def test_stand_alone_program_under_sanitizers(tmp_path):
    """the lane-code driver with its own main, built with -fsanitize=address,undefined and run as a program (never loaded into python)"""
    exe = str(tmp_path / "bf_denoisetest")
    src = os.path.join(bfutil.ROOT, "tests", "hosttest", "bf_denoisetest.cpp")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-DBF_DENOISETEST_MAIN", src, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("denoise ok:"), r.stdout + r.stderr
