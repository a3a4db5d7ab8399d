"""GPU: IdsToRowsBatchDevice / IdsToRowsBatch (bf_kernels_rows.hip) and the Python calls above them against the numpy restatement of
the specification (rows_cases.restate): the parameter table on synthetic ragged ids, the capacity guard over canary-filled buffers,
unaligned outputs, sequence counts around the scan tile, one sequence of very many windows, bad ranges, refused arguments, handles of
every kind, and text -> rows end to end against the stored reference ids (tests/golden/rows/encode_ids.json)."""
import ctypes

import numpy as np
import pytest
import torch

import bfutil
import blingfire_amd as bf
import rows_cases as rc

pytestmark = pytest.mark.gpu

CANARY32, CANARY8 = -0x35014542, 0xA5
E_ARG, E_CAPACITY = -1, -3
vp = ctypes.c_void_p


@pytest.fixture(scope="module")
def h():
    hm = bf.load_model(bfutil.model_path(bfutil.bert_model_name()))
    yield hm
    bf.free_model(hm)


def status(hm):
    torch.cuda.synchronize()
    return bf.lib().BfLastStatus(vp(hm))


def ptr(t):
    return None if t is None else t.data_ptr()


def device_call(hm, d_ids, ids_len, d_off, nseq, L, cls_id, sep_id, pad_id, stride, max_rows, flags, rows, mask, seq, first, cap, r_off):
    return bf.lib().IdsToRowsBatchDevice(vp(hm), ptr(d_ids), ids_len, ptr(d_off), nseq, L, cls_id, sep_id, pad_id, stride, max_rows, flags,
                                         ptr(rows), ptr(mask), ptr(seq), ptr(first), cap, ptr(r_off), None)


def canaries(cap, L, tail=0):
    """canary-filled outputs of cap rows (+ tail elements the call must not touch either)"""
    return (torch.full((cap * L + tail,), CANARY32, dtype=torch.int32, device="cuda"), torch.full((cap * L + tail,), CANARY8, dtype=torch.uint8, device="cuda"),
            torch.full((cap + tail,), CANARY32, dtype=torch.int32, device="cuda"), torch.full((cap + tail,), CANARY32, dtype=torch.int32, device="cuda"))


def check_device(hm, ids, off, par, cap=None, ids_len=None, want_status=None, outs=(True, True, True, True), want=None):
    """one device call over canary-filled buffers of `cap` rows (default: the total): everything below min(cap, total) equals the
    restatement, nothing at or past it changed, the offsets are complete, the status word is what the restatement says"""
    L, cls_id, sep_id, stride, max_rows, pad_left = par
    if want is None:
        want = rc.restate(ids, off, L, cls_id, sep_id, rc.PAD, stride, max_rows, pad_left, ids_len=ids_len)
    total = len(want[2])
    cap = total if cap is None else cap
    d_ids = torch.from_numpy(np.ascontiguousarray(ids, dtype=np.int32)).cuda()
    d_off = torch.from_numpy(np.ascontiguousarray(off, dtype=np.int64)).cuda()
    bufs = canaries(cap, L, tail=64)
    r_off = torch.full((len(off),), -1, dtype=torch.int64, device="cuda")
    use = [b if u else None for b, u in zip(bufs, outs)]
    r = device_call(hm, d_ids, len(ids) if ids_len is None else ids_len, d_off, len(off) - 1, L, cls_id, sep_id, rc.PAD, stride, max_rows, 1 if pad_left else 0,
                    *use, cap, r_off)
    assert r == 0, (par, r)
    st = status(hm)
    k = min(cap, total)
    assert np.array_equal(r_off.cpu().numpy(), want[4]), par
    got = [b.cpu().numpy() for b in bufs]
    for i, (g, w, width, can) in enumerate(zip(got, want[:4], (L, L, 1, 1), (CANARY32, CANARY8, CANARY32, CANARY32))):
        if outs[i]:
            assert np.array_equal(g[:k * width], w[:k].reshape(-1)), (par, cap, i)
            assert (g[k * width:] == can).all(), (par, cap, i)
        else:
            assert (g == can).all(), (par, cap, i)
    dropped = 1 if (total > cap and any(outs)) else 0
    assert st == (want[5] | dropped if want_status is None else want_status), (par, cap, st)
    return want


def check_host(hm, ids, off, par):
    L, cls_id, sep_id, stride, max_rows, pad_left = par
    want = rc.restate(ids, off, L, cls_id, sep_id, rc.PAD, stride, max_rows, pad_left)
    got = bf.ids_to_rows_batch(hm, ids, off, L, cls_id, sep_id, rc.PAD, stride, max_rows, pad_left)
    for g, w in zip(got, want[:5]):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), par


# ---- 1. the parameter table on synthetic ragged ids
@pytest.mark.parametrize("L", rc.TABLE_L)
def test_1_parameter_table(h, L):
    n = 0
    for par in rc.table():
        if par[0] != L:
            continue
        body, step = rc.geometry(L, par[1], par[2], par[3])
        ids, off = rc.synthetic(body, step, seed=n)
        check_device(h, ids, off, par)
        check_host(h, ids, off, par)
        n += 1
    assert n > 0


# ---- 2. capacity
@pytest.mark.parametrize("par", [(8, rc.CLS, rc.SEP, 2, 0, False), (63, rc.CLS, -1, 1, 3, True), (64, rc.CLS, rc.SEP, 0, 0, False)])
def test_2_capacity(h, par):
    L, cls_id, sep_id, stride, max_rows, pad_left = par
    body, step = rc.geometry(L, cls_id, sep_id, stride)
    ids, off = rc.synthetic(body, step)
    total = len(rc.restate(ids, off, L, cls_id, sep_id, rc.PAD, stride, max_rows, pad_left)[2])
    for cap in (0, total - 1, total, total + 1):
        check_device(h, ids, off, par, cap=cap)                   # status bit 0 exactly when total > cap
    # the size query: every output NULL (no drop is reported: nothing was asked for), then each optional output NULL in turn
    check_device(h, ids, off, par, cap=0, outs=(False,) * 4)
    for drop in range(4):
        check_device(h, ids, off, par, outs=tuple(i != drop for i in range(4)))
        check_device(h, ids, off, par, cap=total - 1, outs=tuple(i != drop for i in range(4)))
    # host form: BF_E_CAPACITY, offsets complete, nothing else written
    want = rc.restate(ids, off, L, cls_id, sep_id, rc.PAD, stride, max_rows, pad_left)
    ids = np.ascontiguousarray(ids, dtype=np.int32); off = np.ascontiguousarray(off, dtype=np.int64)
    for cap in (0, total - 1):
        rows = np.full((cap, L), CANARY32, dtype=np.int32); mask = np.full((cap, L), CANARY8, dtype=np.uint8)
        seq = np.full(cap, CANARY32, dtype=np.int32); first = np.full(cap, CANARY32, dtype=np.int32); r_off = np.full(len(off), -1, dtype=np.int64)
        r = bf.lib().IdsToRowsBatch(vp(h), ids.ctypes.data, off.ctypes.data, len(off) - 1, L, cls_id, sep_id, rc.PAD, stride, max_rows, 1 if pad_left else 0,
                                    rows.ctypes.data, mask.ctypes.data, seq.ctypes.data, first.ctypes.data, cap, r_off.ctypes.data)
        assert r == E_CAPACITY and np.array_equal(r_off, want[4])
        assert (rows == CANARY32).all() and (mask == CANARY8).all() and (seq == CANARY32).all() and (first == CANARY32).all()
    r_off = np.full(len(off), -1, dtype=np.int64)
    r = bf.lib().IdsToRowsBatch(vp(h), ids.ctypes.data, off.ctypes.data, len(off) - 1, L, cls_id, sep_id, rc.PAD, stride, max_rows, 1 if pad_left else 0,
                                None, None, None, None, 0, r_off.ctypes.data)
    assert r == total and np.array_equal(r_off, want[4])                  # the size query needs no capacity
    # each output alone, then each left out in turn: what was asked for equals the restatement, nothing else is touched
    cans = (CANARY32, CANARY8, CANARY32, CANARY32)
    for asked in [tuple(i == k for i in range(4)) for k in range(4)] + [tuple(i != k for i in range(4)) for k in range(4)]:
        outs = [np.full((total, L), CANARY32, dtype=np.int32), np.full((total, L), CANARY8, dtype=np.uint8),
                np.full(total, CANARY32, dtype=np.int32), np.full(total, CANARY32, dtype=np.int32)]
        r_off = np.full(len(off), -1, dtype=np.int64)
        r = bf.lib().IdsToRowsBatch(vp(h), ids.ctypes.data, off.ctypes.data, len(off) - 1, L, cls_id, sep_id, rc.PAD, stride, max_rows, 1 if pad_left else 0,
                                    *[o.ctypes.data if a else None for o, a in zip(outs, asked)], total, r_off.ctypes.data)
        assert r == total and np.array_equal(r_off, want[4]), (par, asked)
        assert all(np.array_equal(o, want[i]) if asked[i] else (o == cans[i]).all() for i, o in enumerate(outs)), (par, asked)


# ---- 3. alignment
@pytest.mark.parametrize("L", [64, 63])
@pytest.mark.parametrize("rows_shift,mask_shift", [(0, 0), (1, 0), (0, 1), (1, 1), (2, 2), (4, 4)])
def test_3_alignment(h, L, rows_shift, mask_shift):
    """outputs that start rows_shift elements / mask_shift bytes behind a 16-byte boundary"""
    body, step = rc.geometry(L, rc.CLS, rc.SEP, 3)
    ids, off = rc.synthetic(body, step)
    want = rc.restate(ids, off, L, rc.CLS, rc.SEP, rc.PAD, 3, 0, False)
    total = len(want[2])
    d_ids = torch.from_numpy(ids).cuda(); d_off = torch.from_numpy(off).cuda()
    rows_buf = torch.full((total * L + 64,), CANARY32, dtype=torch.int32, device="cuda")
    mask_buf = torch.full((total * L + 64,), CANARY8, dtype=torch.uint8, device="cuda")
    assert rows_buf.data_ptr() % 16 == 0 and mask_buf.data_ptr() % 16 == 0
    rows, mask = rows_buf[rows_shift:], mask_buf[mask_shift:]
    r_off = torch.empty(len(off), dtype=torch.int64, device="cuda")
    assert device_call(h, d_ids, len(ids), d_off, len(off) - 1, L, rc.CLS, rc.SEP, rc.PAD, 3, 0, 0, rows, mask, None, None, total, r_off) == 0
    assert status(h) == 0
    g_rows, g_mask = rows_buf.cpu().numpy(), mask_buf.cpu().numpy()
    assert np.array_equal(g_rows[rows_shift:rows_shift + total * L], want[0].reshape(-1)) and np.array_equal(g_mask[mask_shift:mask_shift + total * L], want[1].reshape(-1))
    assert (g_rows[:rows_shift] == CANARY32).all() and (g_rows[rows_shift + total * L:] == CANARY32).all()
    assert (g_mask[:mask_shift] == CANARY8).all() and (g_mask[mask_shift + total * L:] == CANARY8).all()


# ---- 4. scan and search edges
def mixed(nseq, seed, longest=40):
    rnd = np.random.RandomState(seed)
    lens = rnd.randint(0, longest, size=nseq)
    lens[rnd.randint(0, nseq, size=max(1, nseq // 50))] = 0
    off = np.zeros(nseq + 1, dtype=np.int64)
    np.cumsum(lens, out=off[1:])
    return (1000 + np.arange(int(off[-1]))).astype(np.int32), off


@pytest.mark.parametrize("nseq", [1, 1023, 1024, 1025, 5000])
def test_4_sequence_counts_around_the_scan_tile(h, nseq):
    ids, off = mixed(nseq, nseq)
    check_device(h, ids, off, (8, rc.CLS, rc.SEP, 2, 0, False))
    check_device(h, ids, off, (12, rc.CLS, rc.SEP, 0, 1, True))
    check_host(h, ids, off, (8, rc.CLS, -1, 3, 2, False))


def test_4_one_sequence_of_very_many_windows(h):
    """200,000 ids at L = 8, stride = 5 (199,995 windows, one id apart) among short sequences; also with neither row_seq nor row_first taken,
    where the fill has workspace for the first rows only and finds the rest by its own search"""
    lens = [3, 0, 7, 200000, 1, 6, 9]
    off = np.zeros(len(lens) + 1, dtype=np.int64); np.cumsum(lens, out=off[1:])
    ids = (1000 + np.arange(int(off[-1]))).astype(np.int32)
    par = (8, rc.CLS, rc.SEP, 5, 0, False)
    want = check_device(h, ids, off, par)
    assert len(want[2]) == 1 + 1 + 2 + (1 + 199994) + 1 + 1 + 4
    check_device(h, ids, off, par, outs=(True, True, False, False), want=want)
    check_device(h, ids, off, (8, -1, -1, 0, 0, True), outs=(True, False, False, True))


# ---- 5. bad ranges
def test_5_bad_ranges(h):
    ids = (1000 + np.arange(60)).astype(np.int32)
    par = (8, rc.CLS, rc.SEP, 2, 0, False)
    for off, ids_len in (([0, 5, 3, 12, 20], 60),             # decreasing
                         ([0, 10, 70, 70, 80], 60),            # a range past ids_len
                         ([0, 10, 20, 35, 60], 30),            # ids_len below id_offsets[nseq]: a tokenizer call that overflowed its ids_cap
                         ([-1, 4, 9], 60)):
        want = check_device(h, ids, np.array(off, dtype=np.int64), par, ids_len=ids_len)
        assert want[5] == 8
        bad = [q for q in range(len(off) - 1) if off[q] < 0 or off[q + 1] < off[q] or off[q + 1] > ids_len]
        for q in bad:                                          # a specials-only row
            r0 = want[4][q]
            assert want[4][q + 1] == r0 + 1 and want[0][r0].tolist() == [rc.CLS, rc.SEP] + [rc.PAD] * 6 and want[1][r0].tolist() == [1, 1] + [0] * 6
    # the host form takes the ids up to the largest offset: decreasing offsets there too
    off = np.array([0, 5, 3, 12, 20], dtype=np.int64)
    want = rc.restate(ids, off, 8, rc.CLS, rc.SEP, rc.PAD, 2, 0, False, ids_len=20)
    got = bf.ids_to_rows_batch(h, ids, off, 8, rc.CLS, rc.SEP, rc.PAD, 2, 0)
    for g, w in zip(got, want[:5]):
        assert np.array_equal(g, w)
    assert bf.lib().BfLastStatus(vp(h)) == 8


def test_5_behind_a_tokenizer_call_that_overflowed(h):
    """TextToIdsBatchDevice with an ids_cap too small, IdsToRowsBatchDevice behind it on the same stream with ids_len = that capacity, no
    synchronisation between them: the documents whose ids did not fit get a specials-only row, the others their exact rows"""
    docs = [b"hello world again", b"unaffable telescope", b"a b c d e f g h i j k l m n o p", b"the end"]
    text, doff = bf.pack_docs(docs)
    full_ids, full_off = bf.text_to_ids_batch(h, (text, doff), 64, 100)
    cap = int(full_off[2]) + 3                                 # documents 0 and 1 fit, 2 and 3 do not
    d_text = torch.from_numpy(text.copy()).cuda(); d_doff = torch.from_numpy(doff).cuda()
    d_ids = torch.full((cap,), -1, dtype=torch.int32, device="cuda")
    d_ids, d_idoff = bf.text_to_ids_batch_device(h, d_text, d_doff, 64, 100, out_ids=d_ids)
    rows, mask, seq, first, r_off = bf.ids_to_rows_batch_device(h, d_ids, d_idoff, 8, rc.CLS, rc.SEP, rc.PAD)
    assert status(h) == 8
    assert np.array_equal(d_idoff.cpu().numpy(), full_off)
    want = rc.restate(full_ids, full_off, 8, rc.CLS, rc.SEP, rc.PAD, 0, 1, False, ids_len=cap)
    for g, w in zip((rows, mask, seq, first, r_off), want[:5]):
        assert np.array_equal(g.cpu().numpy(), w)
    assert want[0][2].tolist() == [rc.CLS, rc.SEP] + [rc.PAD] * 6 and want[0][0][1] == full_ids[0]


# ---- 6. arguments
def test_6_refused_arguments(h):
    ids = torch.arange(4, dtype=torch.int32, device="cuda"); off = torch.tensor([0, 4], dtype=torch.int64, device="cuda")
    r_off = torch.full((2,), -1, dtype=torch.int64, device="cuda")
    ok = dict(L=8, cls_id=1, sep_id=2, pad_id=0, stride=0, max_rows=1, flags=0)

    def call(hm=h, ids_len=4, nseq=1, cap=0, d_off=off, d_r_off=r_off, **kw):
        a = dict(ok, **kw)
        return device_call(hm, ids, ids_len, d_off, nseq, a["L"], a["cls_id"], a["sep_id"], a["pad_id"], a["stride"], a["max_rows"], a["flags"], None, None, None, None, cap, d_r_off)
    assert call() == 0
    for bad in (dict(L=0), dict(L=-3), dict(L=(1 << 20) + 1), dict(L=2), dict(L=1, sep_id=-1), dict(L=1, cls_id=-1), dict(stride=-1), dict(stride=6),
                dict(stride=7), dict(max_rows=-1), dict(flags=2), dict(flags=3), dict(flags=1 << 8), dict(flags=-2)):
        assert call(**bad) == E_ARG, bad
    assert call(L=1, cls_id=-1, sep_id=-1) == 0 and call(L=1 << 20) == 0 and call(stride=5) == 0 and call(flags=1) == 0 and call(pad_id=-7) == 0
    assert call(hm=None) == E_ARG                              # a NULL handle
    assert call(nseq=-1) == E_ARG and call(ids_len=-1) == E_ARG and call(cap=-1) == E_ARG and call(d_off=None) == E_ARG and call(d_r_off=None) == E_ARG
    hi = np.arange(4, dtype=np.int32); ho = np.array([0, 4], dtype=np.int64); hr = np.zeros(2, dtype=np.int64)
    L = bf.lib()
    assert L.IdsToRowsBatch(None, hi.ctypes.data, ho.ctypes.data, 1, 8, 1, 2, 0, 0, 1, 0, None, None, None, None, 0, hr.ctypes.data) == E_ARG
    assert L.IdsToRowsBatch(vp(h), hi.ctypes.data, ho.ctypes.data, 1, 2, 1, 2, 0, 0, 1, 0, None, None, None, None, 0, hr.ctypes.data) == E_ARG
    assert L.IdsToRowsBatch(vp(h), hi.ctypes.data, ho.ctypes.data, 1, 8, 1, 2, 0, 0, 1, 2, None, None, None, None, 0, hr.ctypes.data) == E_ARG
    assert L.IdsToRowsBatch(vp(h), hi.ctypes.data, ho.ctypes.data, 1, 8, 1, 2, 0, 0, 1, 0, None, None, None, None, 0, None) == E_ARG
    neg = np.array([-1, 3], dtype=np.int64)                    # the host form reads ids from id_offsets[0] on: a negative one is refused
    assert L.IdsToRowsBatch(vp(h), hi.ctypes.data, neg.ctypes.data, 1, 8, 1, 2, 0, 0, 1, 0, None, None, None, None, 0, hr.ctypes.data) == E_ARG


def test_6_no_sequences(h):
    off = torch.zeros(1, dtype=torch.int64, device="cuda"); r_off = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    bufs = canaries(4, 8)
    assert device_call(h, None, 0, off, 0, 8, rc.CLS, rc.SEP, rc.PAD, 0, 1, 0, *bufs, 4, r_off) == 0
    assert status(h) == 0 and r_off.cpu().tolist() == [0]
    assert all((b.cpu().numpy() == c).all() for b, c in zip(bufs, (CANARY32, CANARY8, CANARY32, CANARY32)))
    got = bf.ids_to_rows_batch(h, np.zeros(0, dtype=np.int32), np.zeros(1, dtype=np.int64), 8, rc.CLS, rc.SEP)
    assert got[0].shape == (0, 8) and got[1].shape == (0, 8) and len(got[2]) == 0 and len(got[3]) == 0 and got[4].tolist() == [0]


def test_6_handles_of_every_kind():
    import w2h_cases
    ids, off = rc.synthetic(6, 4)
    par = (8, rc.CLS, rc.SEP, 2, 0, False)
    kinds = []
    for path in (bfutil.model_path(bfutil.bert_model_name()), bfutil.model_path("gpt2.bin"), bfutil.model_path("bert_base_tok.i2w"), w2h_cases.FIXTURE):
        hm = bf.load_model(path)
        try:
            kinds.append(bf.lib().BfModelKind(vp(hm)))
            assert bf.lib().BfReserve(vp(hm), 64, 1 << 12, 0) == 0      # every kind: the rows workspaces at least
            check_device(hm, ids, off, par)
            check_host(hm, ids, off, par)
        finally:
            bf.free_model(hm)
    assert kinds == [0, 3, 5, 6]                               # WordPiece, BPE, [i2w] only, [w2h] only


# ---- 7. end to end
@pytest.fixture(scope="module")
def fx():
    return rc.load_fixture()


@pytest.mark.parametrize("model", sorted(rc.ENCODE_MODELS))
@pytest.mark.parametrize("case", rc.ENCODE_CASES)
def test_7_text_to_rows(fx, model, case):
    L, stride, max_rows, pad_left = case
    sp = rc.ENCODE_MODELS[model]
    docs = rc.encode_docs()
    ref_ids, ref_off = rc.fixture_ids(fx, model, rc.encode_max_len(L, stride, max_rows))
    want = rc.restate(ref_ids, ref_off, L, sp["cls_id"], sp["sep_id"], sp["pad_id"], stride, max_rows, pad_left)
    hm = bf.load_model(bfutil.model_path(model))
    try:
        text, off = bf.pack_docs(docs)
        d_text = torch.from_numpy(text.copy()).cuda(); d_off = torch.from_numpy(off).cuda()
        for got in (bf.encode_batch(hm, docs, L, sp["cls_id"], sp["sep_id"], sp["pad_id"], sp["unk"], stride, max_rows, pad_left),
                    bf.encode_batch_device(hm, d_text, d_off, L, sp["cls_id"], sp["sep_id"], sp["pad_id"], sp["unk"], stride, max_rows, pad_left)):
            torch.cuda.synchronize()
            rows, mask, row_doc, r_off = got
            assert rows.dtype == torch.int32 and mask.dtype == torch.uint8 and row_doc.dtype == torch.int32 and r_off.dtype == torch.int64
            assert tuple(rows.shape) == want[0].shape and tuple(mask.shape) == want[1].shape
            assert np.array_equal(rows.cpu().numpy(), want[0]) and np.array_equal(mask.cpu().numpy(), want[1])
            assert np.array_equal(row_doc.cpu().numpy(), want[2]) and np.array_equal(r_off.cpu().numpy(), want[4])
            assert bf.lib().BfLastStatus(vp(hm)) == 0
    finally:
        bf.free_model(hm)


def test_7_repeated_call_after_reserve_allocates_nothing():
    """after BfReserve a repeated encode_batch_device leaves the device's free memory where it was (hipMemGetInfo): torch serves the
    outputs from its cache, the library's workspaces do not grow"""
    docs = rc.encode_docs() * 8
    text, off = bf.pack_docs(docs)
    sp = rc.ENCODE_MODELS["bert_base_tok.bin"]
    hm = bf.load_model(bfutil.model_path("bert_base_tok.bin"))
    try:
        bf.reserve(hm, len(docs), len(text))
        grows0 = bf.workspace_grows()
        d_text = torch.from_numpy(text.copy()).cuda(); d_off = torch.from_numpy(off).cuda()
        a = bf.encode_batch_device(hm, d_text, d_off, 16, sp["cls_id"], sp["sep_id"], sp["pad_id"], sp["unk"])
        torch.cuda.synchronize()
        assert bf.workspace_grows() == grows0, "the FIRST call on the reserved handle made the library allocate device memory (BfWorkspaceGrows)"
        a = [t.cpu().numpy() for t in a]
        free0 = torch.cuda.mem_get_info()[0]
        b = bf.encode_batch_device(hm, d_text, d_off, 16, sp["cls_id"], sp["sep_id"], sp["pad_id"], sp["unk"])
        torch.cuda.synchronize()
        free1 = torch.cuda.mem_get_info()[0]
        assert free1 == free0, "the device's free memory moved by %d bytes across a reserved call" % (free0 - free1)
        assert bf.workspace_grows() == grows0, "the repeated call made the library allocate device memory (BfWorkspaceGrows)"
        for x, y in zip(a, b):
            assert np.array_equal(x, y.cpu().numpy())
    finally:
        bf.free_model(hm)
