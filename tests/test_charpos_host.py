"""CPU tier of the offset conversions (ByteToCharOffsetsBatchDevice / CharToByteOffsetsBatchDevice): the restatement of charpos_cases is held to
Python's own codecs on every valid-UTF-8 case and to B_d(C_d(i)) == i on character boundaries; the table is shown to hold what it is there for;
the lane code of blingfire_amd/csrc/bf_charpos.h, compiled for the host and driven in the kernels' partition (tests/hosttest/bf_charpostest.cpp:
64-byte chunks, masks, P, both searches), equals the restatement on every case, both units, both directions, the four end conventions; the refused
arguments; the symbols are declared and exported and the wrappers carry the new keywords; the stand-alone program under the sanitizers."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import bfutil
import charpos_cases as cc

c_i64, c_int, c_vp = ctypes.c_int64, ctypes.c_int, ctypes.c_void_p


@pytest.fixture(scope="module")
def ht():
    L = ctypes.CDLL(bfutil.HOSTTEST_LIB)
    L.bft_charpos.restype = c_int
    L.bft_charpos.argtypes = [c_int, c_vp, c_vp, c_i64, c_i64, c_vp, c_i64, c_vp, c_vp, c_int, c_int, c_vp, c_vp, c_vp, c_vp]
    L.bft_charpos_index.restype = None
    L.bft_charpos_index.argtypes = [c_vp, c_i64, c_vp, c_vp, c_vp]
    return L


def addr(a):
    return None if a is None else a.ctypes.data


def host_convert(ht, text, doc_off, unit, direction, flags=0, starts=None, ends=None, item_off=None, items_cap=None, want_units=True, in_place=False):
    """one call of the driver over canary-filled outputs -> what charpos_cases.restate returns"""
    buf = np.frombuffer(bytes(text), dtype=np.uint8).copy()
    doc_off = np.ascontiguousarray(doc_off, dtype=np.int64)
    ndocs = len(doc_off) - 1
    given = starts if starts is not None else ends
    cap = (0 if given is None else len(given)) if items_cap is None else items_cap
    outs = [None if a is None else (a.copy() if in_place else np.full(len(a), cc.CANARY32, dtype=np.int32)) for a in (starts, ends)]
    ins = [o if in_place else a for a, o in zip((starts, ends), outs)]
    units = np.full(ndocs, cc.CANARY32, dtype=np.int32) if want_units else None
    status = ctypes.c_int(-1)
    r = ht.bft_charpos(direction, addr(buf) if len(buf) else None, addr(doc_off), ndocs, len(buf), addr(item_off), cap, addr(ins[0]), addr(ins[1]), unit, flags,
                       addr(outs[0]), addr(outs[1]), addr(units), ctypes.byref(status))
    assert r == 0
    return dict(starts=outs[0], ends=outs[1], doc_units=units, status=status.value)


def same(got, want, what, orig=(None, None)):
    n = want["n"]
    for name, src in zip(("starts", "ends"), orig):
        if want[name] is None:
            continue
        assert np.array_equal(got[name][:n], want[name]), (name, what)
        rest = got[name][n:]                                   # items at or past the bound: not written (in place: as they were)
        assert np.array_equal(rest, src[n:]) if src is not None else (rest == cc.CANARY32).all(), (name, "past the bound", what)
    if got["doc_units"] is not None:
        assert np.array_equal(got["doc_units"], want["doc_units"]), ("doc_units", what)
    assert got["status"] == want["status"], ("status", what, got["status"], want["status"])


# ---- (a) the restatement against Python's codecs
def test_a_restatement_equals_the_codecs():
    checked = 0
    for c in cc.table():
        if not c["valid"] or c.get("bad"):
            continue
        for d in range(len(c["doc_off"]) - 1):
            doc, _ = cc.doc_bytes(c["text"], c["doc_off"], d)
            s = doc.decode()
            C0, C1 = cc.c_table(doc, cc.CHAR), cc.c_table(doc, cc.UTF16)
            bounds = [i for i in range(len(doc) + 1) if i == len(doc) or (doc[i] & 0xC0) != 0x80]
            for i in bounds:
                assert C0[i] == len(doc[:i].decode()) and C1[i] == len(doc[:i].decode().encode("utf-16-le")) // 2
                checked += 1
            for C in (C0, C1):
                B = cc.b_table(C)
                assert all(B[C[i]] == i for i in bounds)         # B_d(C_d(i)) == i on character boundaries
                assert len(B) == C[-1] + 1 and B[-1] == len(doc)
            assert C0[-1] == len(s) and C1[-1] == len(s.encode("utf-16-le")) // 2
            b1 = cc.b_table(C1)                                 # an index on a low surrogate: its character's first byte
            for k in range(C1[-1]):
                at = b1[k]
                if doc[at] >= 0xF0 and C1[at] == k - 1:
                    assert b1[k] == b1[k - 1]
    assert checked > 20000


def test_a_the_table_contains_its_claims():
    assert cc.check_table()
    c = cc.case_named("mixed")
    for unit in cc.UNITS:
        for direction in (cc.FWD, cc.INV):
            v, off = cc.items_for(c, unit, direction)
            assert cc.restate(c["text"], c["doc_off"], unit, direction, 0, v, v, off)["status"] == cc.BAD       # the positions beyond the limit set the bit
            v, off = cc.items_for(c, unit, direction, beyond=False)
            for flags in cc.ALL_FLAGS:
                assert cc.restate(c["text"], c["doc_off"], unit, direction, flags, v, cc.ends_for(v, flags), off)["status"] == 0
    low = cc.restate("a\U0001F600b".encode(), [0, 6], cc.UTF16, cc.INV, 0, np.array([0, 1, 2, 3, 4], dtype=np.int32), None, None, 5)
    assert low["n"] == 1                                       # (no item offsets: one item per document)
    inv = cc.b_table(cc.c_table("a\U0001F600b".encode(), cc.UTF16))
    assert inv == [0, 1, 1, 5, 6]


# ---- (b) the lane code against the restatement
@pytest.mark.parametrize("name", cc.SMALL + ["big"])
def test_b_lane_code_equals_the_restatement(ht, name):
    c = cc.case_named(name)
    for unit in cc.UNITS:
        for direction in (cc.FWD, cc.INV):
            for beyond in (True, False) if name != "big" else (True,):
                v, off = cc.items_for(c, unit, direction, beyond)
                for flags in cc.ALL_FLAGS if name != "big" else (0, 3):          # (the large case is there for the tile edge, not for the conventions)
                    e = cc.ends_for(v, flags)
                    want = cc.restate(c["text"], c["doc_off"], unit, direction, flags, v, e, off)
                    assert beyond or c.get("bad") or want["status"] == 0
                    same(host_convert(ht, c["text"], c["doc_off"], unit, direction, flags, v, e, off), want, (name, unit, direction, flags, beyond))


@pytest.mark.parametrize("name", ["mixed", "edge64", "invalid", "docs_without_items", "bad_ranges"])
def test_b_single_outputs_in_place_caps_and_null_offsets(ht, name):
    c = cc.case_named(name)
    ndocs = len(c["doc_off"]) - 1
    for unit in cc.UNITS:
        for direction in (cc.FWD, cc.INV):
            v, off = cc.items_for(c, unit, direction)
            e = cc.ends_for(v, 3)
            what = (name, unit, direction)
            full = cc.restate(c["text"], c["doc_off"], unit, direction, 3, v, e, off)
            for s_, e_ in ((v, None), (None, e)):               # each output alone
                same(host_convert(ht, c["text"], c["doc_off"], unit, direction, 3, s_, e_, off), cc.restate(c["text"], c["doc_off"], unit, direction, 3, s_, e_, off), what)
            same(host_convert(ht, c["text"], c["doc_off"], unit, direction, 3), cc.restate(c["text"], c["doc_off"], unit, direction, 3), what)      # doc_units alone
            same(host_convert(ht, c["text"], c["doc_off"], unit, direction, 3, v, e, off, in_place=True), full, what)
            for cap in (0, 1, len(v) // 2, len(v) - 1):         # items_cap below off[ndocs]
                want = cc.restate(c["text"], c["doc_off"], unit, direction, 3, v, e, off, cap)
                same(host_convert(ht, c["text"], c["doc_off"], unit, direction, 3, v, e, off, cap), want, what + (cap,))
                same(host_convert(ht, c["text"], c["doc_off"], unit, direction, 3, v, e, off, cap, in_place=True), want, what + (cap, "in place"), (v, e))
            one = np.array([(d % 3) - 1 for d in range(ndocs + 2)], dtype=np.int32)      # NULL offsets: item d belongs to document d; two entries too many
            same(host_convert(ht, c["text"], c["doc_off"], unit, direction, 0, one, one), cc.restate(c["text"], c["doc_off"], unit, direction, 0, one, one), what)


def test_b_index_of_shifted_texts(ht):
    """the masks and weights of a text that sits at every byte shift inside a buffer of 0xF0 bytes: nothing of the neighbours is counted"""
    c = cc.case_named("total_193")
    n = len(c["text"])
    nch = (n + 63) // 64
    want = None
    for shift in range(16):
        buf = np.full(n + shift + 64, 0xF0, dtype=np.uint8)
        buf[shift:shift + n] = np.frombuffer(c["text"], dtype=np.uint8)
        lead, four, cnt = np.zeros(nch, dtype=np.uint64), np.zeros(nch, dtype=np.uint64), np.zeros(nch, dtype=np.int32)
        ht.bft_charpos_index(buf.ctypes.data + shift, n, addr(lead), addr(four), addr(cnt))
        got = (lead.tolist(), four.tolist(), cnt.tolist())
        want = want or got
        assert got == want
    w = [cc.weight(b, cc.UTF16) for b in c["text"]]
    assert want[2] == [sum(w[k:k + 64]) for k in range(0, n, 64)]
    assert want[0] == [sum(1 << r for r, x in enumerate(w[k:k + 64]) if x) for k in range(0, n, 64)]


# ---- (c) refused arguments
def test_c_the_call_refuses_what_the_header_lists(ht):
    text = np.frombuffer(b"abcd", dtype=np.uint8).copy()
    off = np.array([0, 2, 4], dtype=np.int64)
    a, b = np.zeros(4, dtype=np.int32), np.zeros(4, dtype=np.int32)
    u = np.zeros(2, dtype=np.int32)

    def call(direction=0, text_=text, off_=off, ndocs=2, total=4, ioff=None, cap=2, s=a, e=a, unit=0, flags=0, so=b, eo=b, units=u):
        return ht.bft_charpos(direction, addr(text_), addr(off_), ndocs, total, addr(ioff), cap, addr(s), addr(e), unit, flags, addr(so), addr(eo), addr(units), None)
    good = [dict(), dict(direction=1), dict(unit=1, flags=3), dict(s=None, so=None), dict(e=None, eo=None), dict(s=None, so=None, e=None, eo=None),
            dict(s=None, so=None, e=None, eo=None, units=None, cap=0), dict(text_=None, total=0, off_=np.zeros(3, dtype=np.int64)), dict(ndocs=0, units=None, s=None, so=None, e=None, eo=None),
            dict(so=a, eo=a)]
    for g in good:
        assert call(**g) == 0, g
    bad = [dict(unit=2), dict(unit=-1), dict(flags=4), dict(flags=-1), dict(ndocs=-1), dict(total=-1), dict(cap=-1), dict(so=None), dict(s=None), dict(eo=None), dict(e=None),
           dict(text_=None), dict(off_=None), dict(s=None, so=None, e=None, eo=None, units=None)]
    for x in bad:
        assert call(**x) == -1, x


# ---- (d) declared and exported; the stand-alone program
def test_d_new_symbols_are_declared_and_exported():
    import blingfire_amd as bf
    hdr = open(os.path.join(bfutil.ROOT, "include", "blingfiretokdll_amd.h")).read()
    exports = open(os.path.join(bfutil.ROOT, "blingfire_amd", "csrc", "exports.map")).read()
    lib = ctypes.CDLL(bf.LIB_PATH)
    for name in ("ByteToCharOffsetsBatchDevice", "CharToByteOffsetsBatchDevice"):
        assert re.search(r"BF_API\s+\w+\s+%s\(" % name, hdr)
        assert re.search(r"^\s*%s;" % name, exports, flags=re.M)
        assert hasattr(lib, name) and name in bf._SIGNATURES
        assert name in hdr[hdr.index("Status word of the last batch call"):hdr.index("BF_API int BfLastStatus")]
    keys = {"starts", "ends", "item_off", "unit", "ends_in_exclusive", "ends_out_exclusive", "items_cap", "stream"}
    for fn in (bf.byte_to_char_offsets_device, bf.char_to_byte_offsets_device):
        assert keys <= set(inspect.signature(fn).parameters)
    for fn in (bf.encode_batch_device, bf.encode_pairs_batch_device, bf.encode_packed_batch_device, bf.encode_qa_batch_device):
        p = inspect.signature(fn).parameters
        assert p["offset_unit"].default == "byte" and p["offset_end"].default == "inclusive" and list(p)[-2:] == ["offset_unit", "offset_end"] or fn is bf.encode_qa_batch_device
    p = inspect.signature(bf.encode_qa_batch_device).parameters
    assert p["answer_unit"].default == "byte" and p["offset_unit"].default == "byte" and p["offset_end"].default == "inclusive"
    for fn, kw in ((bf.encode_batch_device, dict(offset_unit="bytes")), (bf.encode_batch_device, dict(offset_end="exclusive")),
                   (bf.encode_batch_device, dict(offset_unit="char")), (bf.encode_packed_batch_device, dict(offset_unit="utf16"))):
        with pytest.raises(ValueError):                        # an unknown unit; exclusive byte ends; a unit without return_offsets
            fn(0, None, None, 8, 101, 102, 0, **kw)


def test_stand_alone_program_under_sanitizers(tmp_path):
    """the lane-code driver with its own main, built with -fsanitize=address,undefined and run as a program (never loaded into python)"""
    exe = str(tmp_path / "bf_charpostest")
    src = os.path.join(bfutil.ROOT, "tests", "hosttest", "bf_charpostest.cpp")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-DBF_CHARPOSTEST_MAIN", src, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("charpos ok:"), r.stdout + r.stderr


def test_e_array_form_of_the_restatement_equals_the_loop():
    for c in cc.table():
        if c.get("bad") or len(c["doc_off"]) < 2:
            continue
        for unit in cc.UNITS:
            for direction in (cc.FWD, cc.INV):
                v, off = cc.items_for(c, unit, direction)
                for flags in cc.ALL_FLAGS if c["name"] != "big" else (3,):
                    e = cc.ends_for(v, flags)
                    want = cc.restate(c["text"], c["doc_off"], unit, direction, flags, v, e, off)
                    s_, e_, u_, st = cc.restate_array(c["text"], c["doc_off"], unit, direction, flags, v, e, off)
                    assert np.array_equal(s_, want["starts"]) and np.array_equal(e_, want["ends"]) and np.array_equal(u_, want["doc_units"]) and st == want["status"], (
                        c["name"], unit, direction, flags)
