"""GPU: the offset conversions (ByteToCharOffsetsBatchDevice / CharToByteOffsetsBatchDevice; k_char_index, the scan, k_char_docs, k_char_fwd, k_char_inv)
through the C ABI, against the restatement of charpos_cases over canary-filled outputs with a guard behind them: every case of the table (both
units, both directions, the four end conventions, the exhaustive positions and the status bit), each output alone and in place, the text at every
byte shift inside a buffer of 0xF0 bytes with the item arrays at odd element shifts, a second round of every grid-stride loop, a batch of more than
2^31 bytes, no allocation after BfReserve, every refused argument, the call order on one handle, and the Python calls end to end."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import bfutil
import blingfire_amd as bf
import charpos_cases as cc

pytestmark = pytest.mark.gpu

E_ARG = -1
vp = ctypes.c_void_p
I32, I64, U8 = torch.int32, torch.int64, torch.uint8
GUARD = 64
FN = {cc.FWD: "ByteToCharOffsetsBatchDevice", cc.INV: "CharToByteOffsetsBatchDevice"}


@pytest.fixture(scope="module")
def h():
    hm = bf.load_model(bfutil.model_path(bfutil.bert_model_name()))
    yield hm
    bf.free_model(hm)


def ptr(t):
    """the address of a view's first element (data_ptr() of an empty view is 0, which the calls would read as "not given")"""
    return None if t is None else t.untyped_storage().data_ptr() + t.storage_offset() * t.element_size()


def status(hm):
    torch.cuda.synchronize()
    return bf.lib().BfLastStatus(vp(hm))


def dev_text(text, shift=0):
    """the text on the device at byte `shift` of a buffer whose other bytes are 0xF0 (a lead byte of weight 2: a miscounted neighbour shows)"""
    t = np.frombuffer(bytes(text), dtype=np.uint8)
    buf = torch.full((len(t) + shift + 48,), 0xF0, dtype=U8, device="cuda")
    if len(t):
        buf[shift:shift + len(t)] = torch.from_numpy(t.copy()).cuda()
    return buf[shift:shift + len(t)]


def dev_arr(a, dtype, shift=0):
    """an array on the device at element `shift` of a larger buffer"""
    if a is None:
        return None
    a = np.array(a, order="C")                                  # (a copy: the shared reference arrays are read-only)
    buf = torch.zeros(len(a) + shift + 3, dtype=dtype, device="cuda")
    if len(a):
        buf[shift:shift + len(a)] = torch.from_numpy(a).cuda()
    return buf[shift:shift + len(a)]


def canary(n, shift=0):
    return torch.full((n + GUARD + shift,), cc.CANARY32, dtype=I32, device="cuda")[shift:]


def call(hm, direction, d_text, total, d_doc_off, ndocs, d_item_off, cap, d_s, d_e, unit, flags, o_s, o_e, o_u, stream=None):
    return getattr(bf.lib(), FN[direction])(vp(hm) if hm else None, ptr(d_text), ptr(d_doc_off), ndocs, total, ptr(d_item_off), cap, ptr(d_s), ptr(d_e), unit, flags,
                                            ptr(o_s), ptr(o_e), ptr(o_u), stream)


def run(hm, c, unit, direction, flags=0, starts=None, ends=None, item_off=None, items_cap=None, units=True, in_place=False, shift=0, ishift=0):
    """one call over canary-filled outputs with a guard behind them -> dict(starts, ends, doc_units: numpy, guard included; status)"""
    ndocs = len(c["doc_off"]) - 1
    d_text = dev_text(c["text"], shift)
    d_doc_off = dev_arr(c["doc_off"], I64, ishift)
    d_item_off = dev_arr(item_off, I64, ishift)
    given = starts if starts is not None else ends
    cap = (0 if given is None else len(given)) if items_cap is None else items_cap
    ins, outs = [], []
    for a in (starts, ends):
        if a is None:
            ins.append(None); outs.append(None)
        elif in_place:
            t = canary(len(a), ishift)
            t[:len(a)] = torch.from_numpy(np.array(a)).cuda()
            ins.append(t); outs.append(t)
        else:
            ins.append(dev_arr(a, I32, ishift)); outs.append(canary(len(a), ishift))
    o_u = canary(ndocs, ishift) if units else None
    r = call(hm, direction, d_text, len(c["text"]), d_doc_off, ndocs, d_item_off, cap, ins[0], ins[1], unit, flags, outs[0], outs[1], o_u)
    assert r == 0, r
    st = status(hm)
    return dict(starts=None if outs[0] is None else outs[0].cpu().numpy(), ends=None if outs[1] is None else outs[1].cpu().numpy(),
                doc_units=None if o_u is None else o_u.cpu().numpy(), status=st)


def same(got, want, what, orig=(None, None)):
    """exact below the item bound, canaries (in place: the inputs) from there to the end of the guard"""
    n = want["n"]
    for name, src in zip(("starts", "ends"), orig):
        if want[name] is None:
            continue
        g = got[name]
        assert np.array_equal(g[:n], want[name]), (name, what)
        if src is not None:
            assert np.array_equal(g[n:len(src)], src[n:]) and (g[len(src):] == cc.CANARY32).all(), (name, "past the bound", what)
        else:
            assert (g[n:] == cc.CANARY32).all(), (name, "past the bound", what)
    if got["doc_units"] is not None:
        nd = len(want["doc_units"])
        assert np.array_equal(got["doc_units"][:nd], want["doc_units"]) and (got["doc_units"][nd:] == cc.CANARY32).all(), ("doc_units", what)
    assert got["status"] == want["status"], ("status", what, got["status"], want["status"])


@functools.lru_cache(maxsize=None)
def reference(name, unit, direction, flags, beyond=True):
    """computed once, shared by the tests, never changed: (values, ends, item offsets, the restatement's answer)"""
    c = cc.case_named(name)
    v, off = cc.items_for(c, unit, direction, beyond)
    e = cc.ends_for(v, flags)
    for a in (v, e, off):
        a.setflags(write=False)
    return v, e, off, cc.restate(c["text"], c["doc_off"], unit, direction, flags, v, e, off)


# ---- 1. every case of the table
@pytest.mark.parametrize("name", cc.SMALL + ["big"])
def test_1_equals_the_restatement(h, name):
    c = cc.case_named(name)
    for unit in cc.UNITS:
        for direction in (cc.FWD, cc.INV):
            for beyond, flags in [(True, f) for f in (cc.ALL_FLAGS if name != "big" else (0, 3))] + ([(False, 0), (False, 3)] if name != "big" else []):
                v, e, off, want = reference(name, unit, direction, flags, beyond)
                assert beyond or c.get("bad") or want["status"] == 0
                same(run(h, c, unit, direction, flags, v, e, off), want, (name, unit, direction, flags, beyond))


def test_1_the_table_contains_its_claims():
    assert cc.check_table()


# ---- 2. each output alone, in place, the item bound, NULL offsets
@pytest.mark.parametrize("name", ["mixed", "edge64", "invalid", "docs_without_items", "bad_ranges", "no_text"])
def test_2_single_outputs_in_place_caps_and_null_offsets(h, name):
    c = cc.case_named(name)
    ndocs = len(c["doc_off"]) - 1
    R = lambda *a: cc.restate(c["text"], c["doc_off"], *a)
    for unit in cc.UNITS:
        for direction in (cc.FWD, cc.INV):
            v, e, off, full = reference(name, unit, direction, 3)
            what = (name, unit, direction)
            same(run(h, c, unit, direction, 3, v, None, off, units=False), R(unit, direction, 3, v, None, off), what)
            same(run(h, c, unit, direction, 3, None, e, off, units=False), R(unit, direction, 3, None, e, off), what)
            same(run(h, c, unit, direction, 3), R(unit, direction, 3), what)                                    # d_doc_units_out alone
            same(run(h, c, unit, direction, 3, v, e, off, in_place=True), full, what, (v, e))
            for cap in (0, 1, len(v) // 2, len(v) - 1):         # items_cap below off[ndocs]: chaining behind a call that overflowed its capacity
                want = R(unit, direction, 3, v, e, off, cap)
                same(run(h, c, unit, direction, 3, v, e, off, cap), want, what + (cap,))
                same(run(h, c, unit, direction, 3, v, e, off, cap, in_place=True), want, what + (cap, "in place"), (v, e))
            one = np.array([(d % 3) - 1 for d in range(ndocs + 2)], dtype=np.int32)      # NULL offsets: item d belongs to document d; two entries too many
            same(run(h, c, unit, direction, 0, one, one), R(unit, direction, 0, one, one), what)


# ---- 3. pointers
@pytest.mark.parametrize("name", ["edge64", "total_193", "total_255", "invalid"])
def test_3_text_at_every_byte_shift_and_item_arrays_at_odd_shifts(h, name):
    c = cc.case_named(name)
    for unit in cc.UNITS:
        for direction in (cc.FWD, cc.INV):
            v, e, off, want = reference(name, unit, direction, 3)
            for shift in range(16):
                same(run(h, c, unit, direction, 3, v, e, off, shift=shift, ishift=1 + shift % 3), want, (name, unit, direction, shift))


# ---- 4. the grid-stride loops
def test_4_more_than_one_pass_of_every_grid(h):
    """rows_blocks launches at most 8 blocks of 256 lanes per compute unit: more wave tiles of 1024 bytes than that many waves, and more items and
    documents than that many lanes, drive a second round of k_char_index, k_char_docs, k_char_fwd and k_char_inv, with a last round in which
    some waves are past the end"""
    lanes = torch.cuda.get_device_properties(0).multi_processor_count * 8 * 256
    tiles = lanes // 64 + 37
    piece = "é€\U0001F600a".encode()                           # 10 bytes a document
    ndocs = (tiles * 1024) // len(piece) + 1
    assert ndocs > lanes and ndocs * len(piece) > (lanes // 64) * 1024
    text = np.frombuffer(piece * ndocs, dtype=np.uint8)
    doc_off = np.arange(ndocs + 1, dtype=np.int64) * len(piece)
    item_off = np.arange(ndocs + 1, dtype=np.int64) * 2         # two items a document
    n = 2 * ndocs
    assert n > lanes
    rnd = np.random.RandomState(5)
    d_text, d_doc_off, d_item_off = torch.from_numpy(text.copy()).cuda(), torch.from_numpy(doc_off).cuda(), torch.from_numpy(item_off).cuda()
    for unit, direction in ((cc.CHAR, cc.FWD), (cc.UTF16, cc.INV)):
        limit = len(piece) if direction == cc.FWD else (4 if unit == cc.CHAR else 5)
        v = rnd.randint(-1, limit + 1, size=n).astype(np.int32)
        ws, we, wu, wst = cc.restate_array(text, doc_off, unit, direction, 3, v, v, item_off)
        o_s, o_e, o_u = canary(n), canary(n), canary(ndocs)
        assert call(h, direction, d_text, len(text), d_doc_off, ndocs, d_item_off, n, dev_arr(v, I32), dev_arr(v, I32), unit, 3, o_s, o_e, o_u) == 0
        assert status(h) == wst == 0
        for got, want in ((o_s, ws), (o_e, we), (o_u, wu)):
            g = got.cpu().numpy()
            assert np.array_equal(g[:len(want)], want) and (g[len(want):] == cc.CANARY32).all()


# ---- 5. more than 2^31 bytes
def test_5_positions_behind_two_gib_of_text(h):
    """three ASCII documents of 2^30, 2^30 and 64 KiB + 1 bytes: every position of the third converts to itself, in both directions, which needs G
    in 64 bits (G in front of the third document is 2^31).  Allocation and fill of the 2 GiB are the test's cost: about a second on an MI355X."""
    n3 = 65537
    total = (1 << 31) + n3
    d_text = torch.full((total,), ord("a"), dtype=U8, device="cuda")
    d_doc_off = torch.tensor([0, 1 << 30, 1 << 31, total], dtype=I64, device="cuda")
    v = np.arange(-1, n3 + 2, dtype=np.int32)
    want = np.where(v <= n3, v, -1).astype(np.int32)
    d_item_off = torch.tensor([0, 0, 0, len(v)], dtype=I64, device="cuda")
    for direction in (cc.FWD, cc.INV):
        o_s, o_e, o_u = canary(len(v)), canary(len(v)), canary(3)
        assert call(h, direction, d_text, total, d_doc_off, 3, d_item_off, len(v), dev_arr(v, I32), dev_arr(v, I32), cc.UTF16, 3, o_s, o_e, o_u) == 0
        assert status(h) == cc.BAD                             # (the one position beyond the document)
        assert np.array_equal(o_s.cpu().numpy()[:len(v)], want) and np.array_equal(o_e.cpu().numpy()[:len(v)], want)
        assert o_u.cpu().numpy()[:3].tolist() == [1 << 30, 1 << 30, n3]
    del d_text
    torch.cuda.empty_cache()


# ---- 6. no allocation after BfReserve
def test_6_no_allocation_after_reserve():
    c = cc.case_named("big")
    ndocs = len(c["doc_off"]) - 1
    hm = bf.load_model(bfutil.model_path(bfutil.bert_model_name()))
    try:
        v, e, off, want = reference("big", cc.UTF16, cc.FWD, 3)
        d_text, d_doc_off, d_item_off = dev_text(c["text"]), dev_arr(c["doc_off"], I64), dev_arr(off, I64)
        d_v, d_e = dev_arr(v, I32), dev_arr(e, I32)
        o_s, o_e, o_u = canary(len(v)), canary(len(v)), canary(ndocs)
        assert bf.lib().BfReserve(vp(hm), ndocs, len(c["text"]), 0) == 0
        torch.cuda.synchronize()
        before = bf.workspace_grows()
        for direction in (cc.FWD, cc.INV):                     # the first call of either kind
            assert call(hm, direction, d_text, len(c["text"]), d_doc_off, ndocs, d_item_off, len(v), d_v, d_e, cc.UTF16, 3, o_s, o_e, o_u) == 0
            torch.cuda.synchronize()
            assert bf.workspace_grows() == before
        fresh = bf.load_model(bfutil.model_path(bfutil.bert_model_name()))           # (and the counter does see the index: an unreserved handle grows)
        try:
            assert call(fresh, cc.FWD, d_text, len(c["text"]), d_doc_off, ndocs, d_item_off, len(v), d_v, d_e, cc.UTF16, 3, o_s, o_e, o_u) == 0
            torch.cuda.synchronize()
            assert bf.workspace_grows() != before
            assert np.array_equal(o_s.cpu().numpy()[:want["n"]], want["starts"])
        finally:
            bf.free_model(fresh)
    finally:
        bf.free_model(hm)


# ---- 7. refused arguments
def test_7_refused_arguments_leave_the_status_word_alone(h):
    c = cc.case_named("mixed")
    ndocs = len(c["doc_off"]) - 1
    d_text, d_off = dev_text(c["text"]), dev_arr(c["doc_off"], I64)
    a, b, u = torch.full((8,), 99, dtype=I32, device="cuda"), torch.zeros(8, dtype=I32, device="cuda"), torch.zeros(8, dtype=I32, device="cuda")
    total = len(c["text"])

    def call7(hm=h, direction=cc.FWD, text=d_text, off=d_off, nd=ndocs, tot=total, ioff=None, cap=ndocs, s=a, e=a, unit=0, flags=0, so=b, eo=b, units=u):
        return call(hm, direction, text, tot, off, nd, ioff, cap, s, e, unit, flags, so, eo, units)
    assert call7() == 0 and status(h) == cc.BAD                 # (position 99 is beyond every document: the word the refused calls must leave alone)
    bad = [dict(unit=2), dict(unit=-1), dict(flags=4), dict(flags=-1), dict(nd=-1), dict(tot=-1), dict(cap=-1), dict(so=None), dict(s=None), dict(eo=None), dict(e=None),
           dict(text=None), dict(off=None), dict(s=None, so=None, e=None, eo=None, units=None), dict(hm=None)]
    for direction in (cc.FWD, cc.INV):
        for x in bad:
            assert call7(direction=direction, **x) == E_ARG, x
            assert status(h) == cc.BAD, x
    ok = [dict(s=None, so=None), dict(e=None, eo=None), dict(s=None, so=None, e=None, eo=None), dict(s=None, so=None, e=None, eo=None, units=None, cap=0),
          dict(nd=0, units=None, s=None, so=None, e=None, eo=None), dict(text=None, tot=0, off=torch.zeros(ndocs + 1, dtype=I64, device="cuda")), dict(unit=1, flags=3)]
    for x in ok:
        assert call7(**x) == 0, x
    assert call7(s=None, so=None, e=None, eo=None, units=None, cap=0) == 0 and status(h) == 0          # (and a call that does nothing still clears the word)


# ---- 8. call order on one handle
def test_8_tokenizer_convert_tokenizer_rows_on_one_handle():
    docs = ["héllo wörld, naïve café", "the quick brown fox", "日本語のテキスト and more", "\U0001F600 smile \U0001F600"]
    text, off = bf.pack_docs(docs)
    d_text, d_off = torch.from_numpy(text.copy()).cuda(), torch.from_numpy(off).cuda()
    c = dict(text=text.tobytes(), doc_off=off)

    def alone(fn):
        hm = bf.load_model(bfutil.model_path(bfutil.bert_model_name()))
        try:
            out = fn(hm)
            return [t.cpu().numpy().copy() for t in out], status(hm)
        finally:
            bf.free_model(hm)
    tok = lambda hm: bf.text_to_ids_with_offsets_batch_device(hm, d_text, d_off, 64, 100)
    (ids, st, en, id_off), tok_status = alone(tok)
    n = int(id_off[-1])
    far = st.copy(); far[0] = 1000                             # one position beyond its document: the convert call's own bit 3
    d_far, d_en, d_idoff = torch.from_numpy(far).cuda(), torch.from_numpy(en).cuda(), torch.from_numpy(id_off).cuda()
    conv = lambda hm: bf.byte_to_char_offsets_device(hm, d_text, d_off, d_far, d_en, d_idoff, unit="utf16", ends_out_exclusive=True)
    rows = lambda hm: bf.ids_to_rows_batch_device(hm, torch.from_numpy(ids).cuda(), d_idoff, 16, 101, 102, 0)
    conv_alone, conv_status = alone(conv)
    rows_alone, rows_status = alone(rows)
    want = cc.restate(c["text"], off, cc.UTF16, cc.FWD, 2, far[:n], en[:n], id_off)
    assert np.array_equal(conv_alone[0][:n], want["starts"]) and np.array_equal(conv_alone[1][:n], want["ends"]) and conv_status == want["status"] == cc.BAD
    assert tok_status == 0 and rows_status == 0
    hm = bf.load_model(bfutil.model_path(bfutil.bert_model_name()))
    try:
        for fn, (want_out, want_status), upto in ((tok, ((ids, st, en, id_off), 0), n), (conv, (conv_alone, cc.BAD), n), (tok, ((ids, st, en, id_off), 0), n),
                                                  (rows, (rows_alone, 0), None)):
            got = fn(hm)
            assert status(hm) == want_status                   # the last call's own
            for g, w in zip(got, want_out):
                g = g.cpu().numpy()
                assert np.array_equal(g[:upto], w[:upto]) if g.shape == w.shape and g.ndim == 1 and len(g) > len(off) else np.array_equal(g, w)
    finally:
        bf.free_model(hm)


# ---- 9. the Python calls end to end
SENTENCES = ["Zürich ist schön, naïve café déjà vu.", "Привет, мир! Как дела?", "日本語のテキストです。", "emoji \U0001F600 in the middle \U0001F680 and end \U0001F600",
             "plain ascii only", "", "Ελληνικά και English mixed ünïcödé", "a"]


def utf16_len(s):
    return len(s.encode("utf-16-le")) // 2


def check_planes(docs, row_doc, st, en, bst, ben, unit):
    """every cell with a token: the slice of the document by the converted pair is the slice of its bytes by the byte pair"""
    cells = 0
    for r in range(st.shape[0]):
        doc = docs[int(row_doc[r])]
        s16 = doc.decode().encode("utf-16-le")
        for j in range(st.shape[1]):
            if bst[r, j] < 0:
                assert st[r, j] == -1 and en[r, j] == -1
                continue
            piece = doc[bst[r, j]:ben[r, j] + 1].decode()
            got = doc.decode()[st[r, j]:en[r, j]] if unit == "char" else s16[2 * st[r, j]:2 * en[r, j]].decode("utf-16-le")
            assert got == piece, (r, j, got, piece)
            cells += 1
    return cells


@pytest.mark.parametrize("unit", ["char", "utf16"])
def test_9_encode_with_offsets_in_characters(h, unit):
    docs = [s.encode() for s in SENTENCES]
    text, off = bf.pack_docs(docs)
    d_text, d_off = torch.from_numpy(text.copy()).cuda(), torch.from_numpy(off).cuda()
    args = (24, 101, 102, 0, 100)
    base = [t.cpu().numpy() for t in bf.encode_batch_device(h, d_text, d_off, *args, return_offsets=True)]
    got = [t.cpu().numpy() for t in bf.encode_batch_device(h, d_text, d_off, *args, return_offsets=True, offset_unit=unit, offset_end="exclusive")]
    assert status(h) == 0
    assert all(np.array_equal(a, b) and a.dtype == b.dtype for a, b in zip(got[:4], base[:4]))          # the other outputs: byte-identical
    assert check_planes(docs, base[2], got[4], got[5], base[4], base[5], unit) > 30
    assert (got[4] != base[4]).any()                           # (non-ASCII text in front of tokens: the planes do differ from the byte planes)
    # pairs: every side against its own text
    docs_b = docs[1:] + docs[:1]
    tb, ob = bf.pack_docs(docs_b)
    d_tb, d_ob = torch.from_numpy(tb.copy()).cuda(), torch.from_numpy(ob).cuda()
    pargs = (40, 101, 102, 0, 100)
    pbase = [t.cpu().numpy() for t in bf.encode_pairs_batch_device(h, d_text, d_off, d_tb, d_ob, *pargs, return_offsets=True, offsets_a=True)]
    pgot = [t.cpu().numpy() for t in bf.encode_pairs_batch_device(h, d_text, d_off, d_tb, d_ob, *pargs, return_offsets=True, offsets_a=True, offset_unit=unit,
                                                                   offset_end="exclusive")]
    assert all(np.array_equal(a, b) for a, b in zip(pgot[:6], pbase[:6]))
    typ, cells = pbase[2], 0
    for side, side_docs in ((0, docs), (1, docs_b)):
        keep = (typ == side) & (pbase[6] >= 0)
        m = lambda p: np.where(keep, p, -1)
        cells += check_planes(side_docs, pbase[3], m(pgot[6]), m(pgot[7]), m(pbase[6]), m(pbase[7]), unit)
    assert cells > 80
    # packed: a row holds several documents; the cell's document is the one its segment names
    kb = [t.cpu().numpy() for t in bf.encode_packed_batch_device(h, d_text, d_off, 32, 101, 102, 0, 100, return_offsets=True)]
    kg = [t.cpu().numpy() for t in bf.encode_packed_batch_device(h, d_text, d_off, 32, 101, 102, 0, 100, return_offsets=True, offset_unit=unit, offset_end="exclusive")]
    assert all(np.array_equal(a, b) for a, b in zip(kg[:7], kb[:7]))
    seg, first, cells = kb[1], kb[3], 0
    for r in range(int(kb[6][0])):
        for k in range(1, int(seg[r].max()) + 1):
            keep = (seg[r:r + 1] == k) & (kb[7][r:r + 1] >= 0)
            m = lambda p: np.where(keep, p[r:r + 1], -1)
            cells += check_planes(docs, [int(first[r]) + k - 1], m(kg[7]), m(kg[8]), m(kb[7]), m(kb[8]), unit)
    assert cells > 40


def test_9_qa_answers_in_characters(h):
    ctx = ["Zürich, größte Stadt der Schweiz — the answer is here, naïve reader.", "Привет! Ответ: сорок два, not forty-one.", "日本語の答えは四十二です、はい。",
           "\U0001F600\U0001F600 the emoji answer \U0001F680 follows", "no answer in this one"]
    qs = ["where?", "сколько?", "何?", "which?", "none"]
    spans = [("answer is here", ), ("сорок два", ), ("四十二", ), ("\U0001F680", ), None]
    a_char = np.full(len(ctx), -1, dtype=np.int32); z_char = a_char.copy(); a_byte = a_char.copy(); z_byte = a_char.copy()
    for k, sp in enumerate(spans):
        if sp is None:
            continue
        at = ctx[k].index(sp[0])
        a_char[k], z_char[k] = at, at + len(sp[0]) - 1
        a_byte[k] = len(ctx[k][:at].encode()); z_byte[k] = len(ctx[k][:at + len(sp[0])].encode()) - 1        # the host conversion the call replaces
    assert (a_byte[:4] > a_char[:4]).all()                     # non-ASCII text in front of every answer
    tq, oq = bf.pack_docs(qs); tc, oc = bf.pack_docs(ctx)
    dv = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    args = (dv(tq.copy()), dv(oq), dv(tc.copy()), dv(oc), 16, 101, 102, 0, 4, 3, 100)
    want = [t.cpu().numpy() for t in bf.encode_qa_batch_device(h, *args, d_ans_first=dv(a_byte), d_ans_last=dv(z_byte))]
    got = [t.cpu().numpy() for t in bf.encode_qa_batch_device(h, *args, d_ans_first=dv(a_char), d_ans_last=dv(z_char), answer_unit="char")]
    assert status(h) == 0 and len(got) == 10
    assert all(np.array_equal(g, w) for g, w in zip(got, want))
    assert (want[8] != 0).sum() >= 2                           # (the answers are found in rows)
    z16 = np.array([-1 if s is None else utf16_len(ctx[k][:ctx[k].index(s[0]) + len(s[0])]) - 1 for k, s in enumerate(spans)], dtype=np.int32)
    a16 = np.array([-1 if s is None else utf16_len(ctx[k][:ctx[k].index(s[0])]) for k, s in enumerate(spans)], dtype=np.int32)
    g16 = [t.cpu().numpy() for t in bf.encode_qa_batch_device(h, *args, d_ans_first=dv(a16), d_ans_last=dv(z16), answer_unit="utf16", offset_unit="char",
                                                               offset_end="exclusive")]
    assert all(np.array_equal(g, w) for g, w in zip(g16[:6] + g16[8:], want[:6] + want[8:]))
    docs = [c.encode() for c in ctx]
    assert check_planes(docs, want[3], g16[6], g16[7], want[6], want[7], "char") > 30
