"""GPU: IdsToPackedRowsBatchDevice / IdsToPackedRowsBatch (bf_kernels_packed.hip) and the Python calls above them against the sequential
restatement of the specification (packed_cases.restate): the parameter table, the exact-fit boundary, chain lengths around the doubling
rounds and the scan tile, runs of width-0 units, one giant sequence, the capacity guard over canary-filled buffers with every subset of
NULL outputs, unaligned pointers, bad ranges, refused arguments, handles of every kind, the host form, and text -> packed rows end to end
against the stored reference ids (tests/golden/rows/encode_ids.json)."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import bfutil
import blingfire_amd as bf
import packed_cases as pc
import rows_cases as rc

pytestmark = pytest.mark.gpu

CANARY = -0x35014542
E_ARG, E_CAPACITY = -1, -3
C, S, P = pc.CLS, pc.SEP, pc.PAD
ALL = (True,) * 6                  # rows, seg, pos, row_first_seq, seq_row, seq_col
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


def device_call(hm, d_ids, ids_len, d_off, nseq, L, cls, sep, pad, flags, rows, seg, pos, first, cap, seq_row, seq_col, nrows):
    return bf.lib().IdsToPackedRowsBatchDevice(vp(hm), ptr(d_ids), ids_len, ptr(d_off), nseq, L, cls, sep, pad, flags, ptr(rows), ptr(seg), ptr(pos), ptr(first), cap,
                                               ptr(seq_row), ptr(seq_col), ptr(nrows), None)


def canary(n):
    return torch.full((n,), CANARY, dtype=torch.int32, device="cuda")


def check_device(hm, ids, off, L, cls, sep, cap=None, ids_len=None, outs=ALL, want=None):
    """one device call over canary-filled buffers of `cap` rows (default: R) with tail elements the call must not touch: everything below
    min(cap, R) equals the restatement, nothing behind it changed, row_first_seq is written up to index min(R, cap) and no further, the
    per-sequence outputs and R are complete, the status word is what the restatement says"""
    if want is None:
        want = pc.restate(ids, off, L, cls, sep, P, ids_len=ids_len)
    R, nseq, key = want[6], len(off) - 1, (L, cls, sep, cap, outs)
    cap = R if cap is None else cap
    d_ids = torch.from_numpy(np.ascontiguousarray(ids, dtype=np.int32)).cuda()
    d_off = torch.from_numpy(np.ascontiguousarray(off, dtype=np.int64)).cuda()
    sizes = (cap * L, cap * L, cap * L, cap + 1, nseq, nseq)
    bufs = [canary(n + 64) for n in sizes]
    nrows = torch.full((3,), -7, dtype=torch.int64, device="cuda")
    use = [b if u else None for b, u in zip(bufs, outs)]
    r = device_call(hm, d_ids, len(ids) if ids_len is None else ids_len, d_off, nseq, L, cls, sep, P, 0, *use[:4], cap, *use[4:], nrows)
    assert r == 0, key
    st = status(hm)
    assert nrows.cpu().tolist() == [R, -7, -7], key
    k = min(cap, R)
    valid = (k * L, k * L, k * L, k + 1, nseq, nseq)
    for i, (b, w) in enumerate(zip(bufs, want[:6])):
        g = b.cpu().numpy()
        n = valid[i] if outs[i] else 0
        assert np.array_equal(g[:n], w.reshape(-1)[:n]), (key, i)
        assert (g[n:] == CANARY).all(), (key, i)
    assert st == (want[7] | (1 if R > cap and any(outs[:4]) else 0)), (key, st)
    return want


def check_host(hm, ids, off, L, cls, sep):
    want = pc.restate(ids, off, L, cls, sep, P)
    got = bf.ids_to_packed_rows_batch(hm, ids, off, L, cls, sep, P)
    for g, w in zip(got, want[:6]):
        assert g.dtype == np.int32 and g.shape == w.shape and np.array_equal(g, w), (L, cls, sep)


# ---- 1. the parameter table
@pytest.mark.parametrize("L", pc.TABLE_L)
def test_1_parameter_table(h, L):
    n = 0
    for l, cls, sep in pc.table():
        if l != L:
            continue
        ids, off = pc.synthetic(pc.geometry(L, cls, sep), seed=n)
        check_device(h, ids, off, L, cls, sep)
        check_host(h, ids, off, L, cls, sep)
        n += 1
    assert n > 0


# ---- 2. the exact-fit boundary
@pytest.mark.parametrize("L", [8, 64])
def test_2_exact_fit_boundary(h, L):
    ids, off = pc.exact_fit(L)
    want = check_device(h, ids, off, L, -1, -1)
    w = np.diff(off)
    used = [int(w[want[3][r]:want[3][r + 1]].sum()) for r in range(want[6])]
    assert L in used and any(u + int(w[want[3][r + 1]]) == L + 1 for r, u in enumerate(used[:-1]))      # W[e] - W[s] == L, and == L + 1


# ---- 3. chain lengths around the doubling rounds (and sequence counts around the scan tile)
@pytest.mark.parametrize("nseq", [1, 2, 3, 4, 5, 63, 64, 65, 1023, 1024, 1025, 5000])
def test_3_chain_lengths(h, nseq):
    ids, off = pc.ragged([4] * nseq)                      # every unit fills a row: R = nseq, the longest chain there is
    want = check_device(h, ids, off, 4, -1, -1)
    assert want[6] == nseq
    ids, off = pc.mixed(nseq, nseq, 12, C, S)
    check_device(h, ids, off, 12, C, S)
    ids, off = pc.mixed(nseq, nseq + 1, 7, -1, S)
    check_device(h, ids, off, 7, -1, S)
    check_host(h, ids, off, 7, -1, S)


# ---- 4. runs of width-0 units, one giant sequence
def test_4_width_zero_runs(h):
    ids, off = pc.ragged([3] + [0] * 100000 + [2])
    want = check_device(h, ids, off, 8, -1, -1)
    assert want[6] == 1 and want[1][0].tolist() == [1, 1, 1, 100002, 100002, 0, 0, 0]
    want = check_device(h, ids, off, 8, C, S)             # width 2 each: four to a row
    assert want[6] == 1 + 25000 + 1


def test_4_one_giant_sequence(h):
    ids, off = pc.ragged([3, 0, 7, 200000, 1, 6, 9])
    want = check_device(h, ids, off, 8, C, S)
    assert want[0][want[4][3]].tolist() == [C] + ids[10:16].tolist() + [S]       # truncated to body
    check_device(h, ids, off, 64, -1, -1)
    check_host(h, ids, off, 8, C, S)


# ---- 5. capacity and NULL outputs
@pytest.mark.parametrize("L,cls,sep", [(8, C, S), (5, C, -1), (64, C, S)])
def test_5_capacity(h, L, cls, sep):
    ids, off = pc.mixed(90, 5 + L, L, cls, sep)
    want = pc.restate(ids, off, L, cls, sep, P)
    R = want[6]
    assert R > 4
    for cap in (0, 1, R - 1, R, R + 3):
        check_device(h, ids, off, L, cls, sep, cap=cap, want=want)      # status bit 0 exactly when R > cap


def test_5_every_subset_of_null_outputs(h):
    ids, off = pc.mixed(40, 11, 8, C, S)
    want = pc.restate(ids, off, 8, C, S, P)
    for outs in itertools.product((False, True), repeat=6):
        check_device(h, ids, off, 8, C, S, outs=outs, want=want)
        check_device(h, ids, off, 8, C, S, cap=want[6] - 1, outs=outs, want=want)     # the size query reports no drop: nothing was asked for


# ---- 6. alignment
@pytest.mark.parametrize("L", [8, 7])
@pytest.mark.parametrize("shifts", [(0, 0, 0), (1, 0, 0), (0, 2, 0), (0, 0, 3), (1, 2, 3), (3, 3, 3), (2, 1, 0), (0, 3, 1)])
def test_6_alignment(h, L, shifts):
    """each plane `shift` elements behind a 16-byte boundary; the ids one element, the offsets one element into larger buffers"""
    ids, off = pc.mixed(50, 17, L, C, S)
    want = pc.restate(ids, off, L, C, S, P)
    R, nseq = want[6], len(off) - 1
    ids_buf = torch.full((len(ids) + 9,), 777777, dtype=torch.int32, device="cuda"); ids_buf[1:1 + len(ids)] = torch.from_numpy(ids).cuda()
    off_buf = torch.full((len(off) + 5,), -5, dtype=torch.int64, device="cuda"); off_buf[1:1 + len(off)] = torch.from_numpy(off).cuda()
    bufs = [canary(R * L + 64) for _ in range(3)]
    assert all(b.data_ptr() % 16 == 0 for b in bufs)
    planes = [b[s:] for b, s in zip(bufs, shifts)]
    nrows = torch.zeros(1, dtype=torch.int64, device="cuda")
    assert device_call(h, ids_buf[1:], len(ids), off_buf[1:], nseq, L, C, S, P, 0, *planes, None, R, None, None, nrows) == 0
    assert status(h) == 0 and int(nrows.item()) == R
    for b, s, w in zip(bufs, shifts, want[:3]):
        g = b.cpu().numpy()
        assert np.array_equal(g[s:s + R * L], w.reshape(-1)) and (g[:s] == CANARY).all() and (g[s + R * L:] == CANARY).all(), (L, shifts)


# ---- 7. bad ranges
def test_7_bad_ranges(h):
    ids = (1000 + np.arange(60)).astype(np.int32)
    for off, ids_len in (([0, 5, 3, 12, 20], 60),             # decreasing
                         ([0, 10, 70, 70, 80], 60),            # a range past ids_len
                         ([0, 10, 20, 35, 60], 30),            # ids_len below id_offsets[nseq]: a tokenizer call that overflowed its ids_cap
                         ([-1, 4, 9], 60)):
        off = np.array(off, dtype=np.int64)
        want = check_device(h, ids, off, 8, C, S, ids_len=ids_len)
        assert want[7] == 8
        for q in range(len(off) - 1):
            r, c = want[4][q], want[5][q]
            if off[q] < 0 or off[q + 1] < off[q] or off[q + 1] > ids_len:      # read as empty: its specials only
                assert want[0][r][c:c + 2].tolist() == [C, S] and (c + 2 == 8 or want[2][r][c + 2] == 0)
            else:                                                               # neighbours intact
                k = min(int(off[q + 1] - off[q]), 6)
                assert want[0][r][c:c + k + 2].tolist() == [C] + ids[off[q]:off[q] + k].tolist() + [S]
    # the host form takes the ids up to the largest offset: decreasing offsets there too
    off = np.array([0, 5, 3, 12, 20], dtype=np.int64)
    want = pc.restate(ids, off, 8, C, S, P, ids_len=20)
    got = bf.ids_to_packed_rows_batch(h, ids, off, 8, C, S, P)
    assert all(np.array_equal(g, w) for g, w in zip(got, want[:6])) and bf.lib().BfLastStatus(vp(h)) == 8


def test_7_behind_a_tokenizer_call_that_overflowed(h):
    """TextToIdsBatchDevice with an ids_cap too small, the packed call behind it on the same stream with ids_len = that capacity and no
    synchronisation between them: the documents whose ids did not fit contribute their specials only, the others their exact units"""
    docs = [b"hello world again", b"unaffable telescope", b"a b c d e f g h i j k l m n o p", b"the end"]
    text, doff = bf.pack_docs(docs)
    full_ids, full_off = bf.text_to_ids_batch(h, (text, doff), 64, 100)
    cap = int(full_off[2]) + 3                                 # documents 0 and 1 fit, 2 and 3 do not
    d_text = torch.from_numpy(text.copy()).cuda(); d_doff = torch.from_numpy(doff).cuda()
    d_ids = torch.full((cap,), -1, dtype=torch.int32, device="cuda")
    d_ids, d_idoff = bf.text_to_ids_batch_device(h, d_text, d_doff, 64, 100, out_ids=d_ids)
    got = bf.ids_to_packed_rows_batch_device(h, d_ids, d_idoff, 16, C, S, P, rows_cap=4)
    assert status(h) == 8
    want = pc.restate(full_ids, full_off, 16, C, S, P, ids_len=cap)
    R = want[6]
    assert R <= 4 and int(got[6].item()) == R
    for g, w in zip(got[:3], want[:3]):
        assert np.array_equal(g.cpu().numpy()[:R], w)
    assert np.array_equal(got[3].cpu().numpy()[:R + 1], want[3]) and np.array_equal(got[4].cpu().numpy(), want[4]) and np.array_equal(got[5].cpu().numpy(), want[5])
    c = want[5][2]
    assert want[0][want[4][2]][c:c + 2].tolist() == [C, S] and want[0][0][1] == full_ids[0]


# ---- 8. arguments
def test_8_refused_arguments(h):
    ids = torch.arange(4, dtype=torch.int32, device="cuda"); off = torch.tensor([0, 4], dtype=torch.int64, device="cuda")
    nrows = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    ok = dict(L=8, cls=1, sep=2, pad=0, flags=0)

    def call(hm=h, d_ids=ids, ids_len=4, nseq=1, cap=0, d_off=off, d_nrows=nrows, **kw):
        a = dict(ok, **kw)
        return device_call(hm, d_ids, ids_len, d_off, nseq, a["L"], a["cls"], a["sep"], a["pad"], a["flags"], None, None, None, None, cap, None, None, d_nrows)
    assert call() == 0 and status(h) == 0 and nrows.item() == 1
    for bad in (dict(L=0), dict(L=-3), dict(L=(1 << 20) + 1), dict(L=2), dict(L=1, sep=-1), dict(L=1, cls=-1), dict(flags=1), dict(flags=2), dict(flags=-1), dict(flags=1 << 8)):
        assert call(**bad) == E_ARG, bad
    assert call(L=1, cls=-1, sep=-1) == 0 and call(L=1 << 20) == 0 and call(pad=-7) == 0 and call(L=3) == 0
    assert call(hm=None) == E_ARG                              # a NULL handle
    assert call(nseq=-1) == E_ARG and call(nseq=1 << 31) == E_ARG and call(cap=-1) == E_ARG and call(d_off=None) == E_ARG and call(d_nrows=None) == E_ARG
    assert call(d_ids=None) == E_ARG and call(ids_len=-1) == E_ARG
    assert call(d_ids=None, ids_len=0) == 0 and status(h) == 8      # no ids may be read: the sequence is outside [0, 0]
    hi = np.arange(4, dtype=np.int32); ho = np.array([0, 4], dtype=np.int64)
    f = bf.lib().IdsToPackedRowsBatch
    tail = (None, None, None, None, 0, None, None)
    assert f(vp(h), hi.ctypes.data, ho.ctypes.data, 1, 8, 1, 2, 0, 0, *tail) == 1
    assert f(None, hi.ctypes.data, ho.ctypes.data, 1, 8, 1, 2, 0, 0, *tail) == E_ARG
    assert f(vp(h), hi.ctypes.data, ho.ctypes.data, 1, 2, 1, 2, 0, 0, *tail) == E_ARG
    assert f(vp(h), hi.ctypes.data, ho.ctypes.data, 1, 8, 1, 2, 0, 1, *tail) == E_ARG
    assert f(vp(h), hi.ctypes.data, None, 1, 8, 1, 2, 0, 0, *tail) == E_ARG
    assert f(vp(h), None, ho.ctypes.data, 1, 8, 1, 2, 0, 0, *tail) == E_ARG
    assert f(vp(h), hi.ctypes.data, ho.ctypes.data, -1, 8, 1, 2, 0, 0, *tail) == E_ARG
    assert f(vp(h), hi.ctypes.data, ho.ctypes.data, 1, 8, 1, 2, 0, 0, None, None, None, None, -1, None, None) == E_ARG
    neg = np.array([-1, 3], dtype=np.int64)                    # the host form reads ids from id_offsets[0] on: a negative one is refused
    assert f(vp(h), hi.ctypes.data, neg.ctypes.data, 1, 8, 1, 2, 0, 0, *tail) == E_ARG


def test_8_no_sequences(h):
    off = torch.zeros(1, dtype=torch.int64, device="cuda")
    want = pc.restate([], [0], 8, C, S, P)
    assert want[6] == 0 and want[3].tolist() == [0]
    check_device(h, np.zeros(0, dtype=np.int32), np.zeros(1, dtype=np.int64), 8, C, S, cap=4, want=want)      # R = 0; row_first_seq[0] = nseq = 0 is the one entry written
    nrows = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    assert device_call(h, None, 0, off, 0, 8, C, S, P, 0, None, None, None, None, 0, None, None, nrows) == 0 and status(h) == 0 and nrows.item() == 0
    got = bf.ids_to_packed_rows_batch(h, np.zeros(0, dtype=np.int32), np.zeros(1, dtype=np.int64), 8, C, S)
    assert [g.shape for g in got] == [(0, 8)] * 3 + [(1,), (0,), (0,)] and got[3].tolist() == [0]


def test_8_handles_of_every_kind():
    import w2h_cases
    ids, off = pc.synthetic(6)
    kinds = []
    for path in (bfutil.model_path(bfutil.bert_model_name()), bfutil.model_path("gpt2.bin"), bfutil.model_path("bert_base_tok.i2w"), w2h_cases.FIXTURE):
        hm = bf.load_model(path)
        try:
            kinds.append(bf.lib().BfModelKind(vp(hm)))
            assert bf.lib().BfReserve(vp(hm), 64, 1 << 12, 0) == 0      # every kind: the packed workspaces too
            check_device(hm, ids, off, 8, C, S)
            check_host(hm, ids, off, 8, C, S)
        finally:
            bf.free_model(hm)
    assert kinds == [0, 3, 5, 6]                               # WordPiece, BPE, [i2w] only, [w2h] only


# ---- 9. the host form
def test_9_host_form(h):
    L = 8
    ids, off = pc.mixed(70, 23, L, C, S)
    ids = np.ascontiguousarray(ids, dtype=np.int32); off = np.ascontiguousarray(off, dtype=np.int64)
    want = pc.restate(ids, off, L, C, S, P)
    R, nseq = want[6], len(off) - 1
    f = bf.lib().IdsToPackedRowsBatch
    pre = (vp(h), ids.ctypes.data, off.ctypes.data, nseq, L, C, S, P, 0)
    # equals the device form (both equal the restatement)
    check_host(h, ids, off, L, C, S)
    check_device(h, ids, off, L, C, S, want=want)
    # the size query needs no capacity, with and without the per-sequence outputs
    assert f(*pre, None, None, None, None, 0, None, None) == R
    seq = [np.full(nseq, CANARY, dtype=np.int32) for _ in range(2)]
    assert f(*pre, None, None, None, None, 0, seq[0].ctypes.data, seq[1].ctypes.data) == R
    assert np.array_equal(seq[0], want[4]) and np.array_equal(seq[1], want[5])
    # BF_E_CAPACITY: the sequence outputs complete, nothing else written
    for cap in (0, R - 1):
        planes = [np.full((cap, L), CANARY, dtype=np.int32) for _ in range(3)]
        first = np.full(cap + 1, CANARY, dtype=np.int32)
        seq = [np.full(nseq, CANARY, dtype=np.int32) for _ in range(2)]
        assert f(*pre, *[p.ctypes.data for p in planes], first.ctypes.data, cap, seq[0].ctypes.data, seq[1].ctypes.data) == E_CAPACITY
        assert all((p == CANARY).all() for p in planes) and (first == CANARY).all()
        assert np.array_equal(seq[0], want[4]) and np.array_equal(seq[1], want[5])
    # each row output alone in buffers larger than needed: what was asked for equals the restatement, nothing else is touched
    for k in range(4):
        planes = [np.full((R + 2, L), CANARY, dtype=np.int32) for _ in range(3)]
        first = np.full(R + 3, CANARY, dtype=np.int32)
        outs = planes + [first]
        assert f(*pre, *[o.ctypes.data if i == k else None for i, o in enumerate(outs)], R + 2, None, None) == R
        for i, o in enumerate(outs):
            n = 0 if i != k else R + 1 if i == 3 else R
            assert np.array_equal(o[:n], want[i][:n]) and (o[n:] == CANARY).all(), (k, i)


# ---- 10. end to end
@pytest.fixture(scope="module")
def fx():
    return rc.load_fixture()


@pytest.mark.parametrize("model", sorted(rc.ENCODE_MODELS))
@pytest.mark.parametrize("L", [16, 8])
def test_10_text_to_packed_rows(fx, model, L):
    sp = rc.ENCODE_MODELS[model]
    docs = rc.encode_docs()
    ref_ids, ref_off = rc.fixture_ids(fx, model, L - 2)       # the stored reference ids at max_len = body
    want = pc.restate(ref_ids, ref_off, L, sp["cls_id"], sp["sep_id"], sp["pad_id"])
    R = want[6]
    assert R < len(docs)                                      # it packs
    hm = bf.load_model(bfutil.model_path(model))
    try:
        text, off = bf.pack_docs(docs)
        d_text = torch.from_numpy(text.copy()).cuda(); d_off = torch.from_numpy(off).cuda()
        for got in (bf.encode_packed_batch(hm, docs, L, sp["cls_id"], sp["sep_id"], sp["pad_id"], sp["unk"]),
                    bf.encode_packed_batch_device(hm, d_text, d_off, L, sp["cls_id"], sp["sep_id"], sp["pad_id"], sp["unk"])):
            torch.cuda.synchronize()
            assert all(t.dtype == torch.int32 for t in got[:6]) and got[6].dtype == torch.int64 and int(got[6].item()) == R
            assert [tuple(t.shape) for t in got[:6]] == [(R, L)] * 3 + [(R + 1,), (len(docs),), (len(docs),)]
            for g, w in zip(got[:6], want[:6]):
                assert np.array_equal(g.cpu().numpy(), w)
            assert bf.lib().BfLastStatus(vp(hm)) == 0
    finally:
        bf.free_model(hm)


def test_10_repeated_call_after_reserve_allocates_nothing():
    """after BfReserve a repeated encode_packed_batch_device with a caller's rows_cap (nothing is read back) leaves the device's free memory
    where it was: torch serves the outputs from its cache, the library's workspaces do not grow.  It gives identical tensors."""
    docs = rc.encode_docs() * 8
    text, off = bf.pack_docs(docs)
    sp = rc.ENCODE_MODELS["bert_base_tok.bin"]
    hm = bf.load_model(bfutil.model_path("bert_base_tok.bin"))
    try:
        bf.reserve(hm, len(docs), len(text))
        grows0 = bf.workspace_grows()
        d_text = torch.from_numpy(text.copy()).cuda(); d_off = torch.from_numpy(off).cuda()
        a = bf.encode_packed_batch_device(hm, d_text, d_off, 16, sp["cls_id"], sp["sep_id"], sp["pad_id"], sp["unk"], rows_cap=len(docs))
        torch.cuda.synchronize()
        assert bf.workspace_grows() == grows0, "the FIRST call on the reserved handle made the library allocate device memory (BfWorkspaceGrows)"
        R = int(a[6].item())
        assert 0 < R < len(docs)
        a = [t.cpu().numpy() for t in a]
        free0 = torch.cuda.mem_get_info()[0]
        b = bf.encode_packed_batch_device(hm, d_text, d_off, 16, sp["cls_id"], sp["sep_id"], sp["pad_id"], sp["unk"], rows_cap=len(docs))
        torch.cuda.synchronize()
        free1 = torch.cuda.mem_get_info()[0]
        assert free1 == free0, "the device's free memory moved by %d bytes across a reserved call" % (free0 - free1)
        assert bf.workspace_grows() == grows0, "the repeated call made the library allocate device memory (BfWorkspaceGrows)"
        for i, (x, y) in enumerate(zip(a, b)):
            n = R if i < 3 else R + 1 if i == 3 else len(x)
            assert np.array_equal(x[:n], y.cpu().numpy()[:n])
    finally:
        bf.free_model(hm)
