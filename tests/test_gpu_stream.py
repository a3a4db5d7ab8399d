"""GPU: IdsToStreamRowsBatchDevice / IdsToStreamRowsBatch (bf_kernels_stream.hip) and the Python calls above them against the restatements of
the specification (stream_cases): the parameter table with all flag values, the tile cases built from the kernel's constants, sequence counts
around the scan tile, streams around one row, one giant sequence, the longest row, the capacity guard over canary-filled buffers with every
subset of NULL outputs, unaligned pointers, bad ranges, chaining behind a tokenizer call that overflowed, refused arguments, handles of every
kind, no allocation after BfReserve, text -> stream rows end to end against the stored reference ids (tests/golden/rows/encode_ids.json), and
the MLM call over the stream rows."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import bfutil
import blingfire_amd as bf
import packed_cases as pc
import rows_cases as rc
import stream_cases as sc

pytestmark = pytest.mark.gpu

CANARY = sc.CANARY
E_ARG, E_CAPACITY = -1, -3
B, E, P, IGN = sc.BOS, sc.EOS, sc.PAD, sc.IGN
ALL = (True,) * 8                  # rows, seg, pos, labels, row_first_seq, row_first_pos, seq_row, seq_col
vp = ctypes.c_void_p


@pytest.fixture(scope="module")
def h():
    hm = bf.load_model(bfutil.model_path("gpt2.bin"))
    yield hm
    bf.free_model(hm)


def status(hm):
    torch.cuda.synchronize()
    return bf.lib().BfLastStatus(vp(hm))


def ptr(t):
    return None if t is None else t.data_ptr()


def device_call(hm, d_ids, ids_len, d_off, nseq, L, bos, eos, pad, ign, flags, outs6, cap, seq_row, seq_col, nrows):
    return bf.lib().IdsToStreamRowsBatchDevice(vp(hm), ptr(d_ids), ids_len, ptr(d_off), nseq, L, bos, eos, pad, ign, flags, *[ptr(t) for t in outs6], cap,
                                               ptr(seq_row), ptr(seq_col), ptr(nrows), None)


def canary(n):
    return torch.full((n,), CANARY, dtype=torch.int32, device="cuda")


def check_device(hm, ids, off, L, bos, eos, flags=0, cap=None, ids_len=None, outs=ALL, want=None, big=False):
    """one device call over canary-filled buffers of `cap` rows (default: R) with tail elements the call must not touch: everything below
    min(cap, R) equals the restatement, nothing behind it changed, the per-sequence outputs and {R, T} are complete, the status word is what the
    restatement says"""
    if want is None:
        want = (sc.restate_np if big else sc.restate)(ids, off, L, bos, eos, P, IGN, flags, ids_len=ids_len)
    R, T, nseq, key = want[8], want[9], len(off) - 1, (L, bos, eos, flags, cap, outs)
    cap = R if cap is None else cap
    d_ids = torch.from_numpy(np.ascontiguousarray(ids, dtype=np.int32)).cuda()
    d_off = torch.from_numpy(np.ascontiguousarray(off, dtype=np.int64)).cuda()
    sizes = [cap * L] * 4 + [cap] * 2 + [nseq] * 2
    bufs = [canary(n + 64) for n in sizes]
    nrows = torch.full((4,), -7, dtype=torch.int64, device="cuda")
    use = [b if u else None for b, u in zip(bufs, outs)]
    r = device_call(hm, d_ids, len(ids) if ids_len is None else ids_len, d_off, nseq, L, bos, eos, P, IGN, flags, use[:6], cap, use[6], use[7], nrows)
    assert r == 0, key
    st = status(hm)
    assert nrows.cpu().tolist() == [R, T, -7, -7], key
    k = min(cap, R)
    valid = [k * L] * 4 + [k] * 2 + [nseq] * 2
    for i, (b, w) in enumerate(zip(bufs, want[:8])):
        g = b.cpu().numpy()
        n = valid[i] if outs[i] else 0
        assert np.array_equal(g[:n], w.reshape(-1)[:n]), (key, sc.NAMES[i])
        assert (g[n:] == CANARY).all(), (key, sc.NAMES[i])
    assert st == (want[10] | (1 if R > cap and any(outs[:6]) else 0)), (key, st)
    return want


def check_host(hm, ids, off, L, bos, eos, flags=0):
    want = sc.restate(ids, off, L, bos, eos, P, IGN, flags)
    got = bf.ids_to_stream_rows_batch(hm, ids, off, L, None if bos < 0 else bos, None if eos < 0 else eos, P, IGN, bool(flags & 1), bool(flags & 2), bool(flags & 4))
    for g, w in zip(got, want[:8]):
        assert g.dtype == np.int32 and g.shape == w.shape and np.array_equal(g, w), (L, bos, eos, flags)


# ---- 1. the parameter table, the worked example
def test_1_worked_example(h):
    ids = np.arange(1000, 1010, dtype=np.int32)
    off = np.array([0, 3, 3, 3, 10], dtype=np.int64)
    want = check_device(h, ids, off, 4, 1, 2)
    assert want[8:10] == (5, 18) and want[0][1].tolist() == [2, 1, 2, 1] and want[3][4].tolist() == [2, -100, -100, -100]
    check_host(h, ids, off, 4, 1, 2)


@pytest.mark.parametrize("L", sc.TABLE_L)
def test_1_parameter_table(h, L):
    n = 0
    for (l, bos, eos, flags) in sc.table():
        if l != L:
            continue
        ids, off = pc.mixed(150, n, max(L, 4))
        check_device(h, ids, off, L, bos, eos, flags)
        if flags in (0, 7):
            check_host(h, ids, off, L, bos, eos, flags)
        n += 1
    assert n == 32


@pytest.mark.parametrize("L", [4, 5, 64])
def test_1_exact_fit_and_ragged(h, L):
    ids, off = pc.exact_fit(max(L, 4))
    check_device(h, ids, off, L, -1, -1)
    check_device(h, ids, off, L, B, E, 7)
    ids, off = pc.ragged([3, 0, 7, 5000, 1, 6, 9])
    check_device(h, ids, off, L, B, E, 4)


# ---- 2. the tile
@pytest.mark.parametrize("wide", [True, False])
def test_2_tile_cases(h, wide):
    g = (ctypes.c_int * 4)()
    ctypes.CDLL(bfutil.HOSTTEST_LIB).bft_stream_geometry(g)   # the tile constants of bf_stream.h: lanes of a tile, cells a wide lane takes, staged units
    lanes, stage = g[0], g[2]
    assert g[1] == 4
    for name, lens, L, bos, eos in sc.tile_cases(lanes * (4 if wide else 1), stage, wide):
        ids, off = sc.ragged(lens)
        want = sc.restate_np(ids, off, L, bos, eos, P, IGN, 0)
        check_device(h, ids, off, L, bos, eos, want=want)
        check_device(h, ids, off, L, bos, eos, 7, big=True)


@pytest.mark.parametrize("nseq", [1, 2, 63, 64, 65, 1023, 1024, 1025, 5000])
def test_2_sequence_counts_around_the_scan_tile(h, nseq):
    ids, off = pc.mixed(nseq, nseq, 12)
    check_device(h, ids, off, 12, B, E, big=True)
    ids, off = pc.mixed(nseq, nseq + 1, 7)
    check_device(h, ids, off, 7, -1, E, 2, big=True)
    check_host(h, ids, off, 7, -1, E, 2)


@pytest.mark.parametrize("L", [4, 5])
def test_2_streams_around_one_row(h, L):
    """T in {0, 1, L - 1, L, L + 1}, with and without the dropped tail: R = 0 writes nothing, {R, T} is always right"""
    for T in (0, 1, L - 1, L, L + 1):
        for flags in (0, 1):
            ids, off = sc.ragged([0, T, 0])
            want = check_device(h, ids, off, L, -1, -1, flags, cap=3)
            assert want[9] == T and want[8] == (T // L if flags else -(-T // L))
            check_host(h, ids, off, L, -1, -1, flags)


def test_2_width_zero_runs(h):
    ids, off = sc.ragged([3] + [0] * 100000 + [2])
    want = check_device(h, ids, off, 8, -1, -1, big=True)
    assert want[8] == 1 and want[1][0].tolist() == [1, 1, 1, 100002, 100002, 0, 0, 0]
    want = check_device(h, ids, off, 8, B, E, big=True)          # width 2 each
    assert want[9] == 2 * 100002 + 5


@pytest.mark.parametrize("L", [8, 4096 + 4])
def test_2_one_giant_sequence(h, L):
    """the one case packed rows cannot express: a sequence of 200,000 ids among small ones, none of it dropped"""
    ids, off = sc.ragged([3, 0, 7, 200000, 1, 6, 9])
    want = check_device(h, ids, off, L, B, E, big=True)
    flat = want[0].reshape(-1)
    assert np.array_equal(flat[flat >= 1000], ids)                # every id, in order
    check_device(h, ids, off, L, -1, -1, 6, big=True)
    if L == 8:
        got = bf.ids_to_stream_rows_batch(h, ids, off, L, B, E, P)
        assert all(np.array_equal(g, w) for g, w in zip(got, want[:8]))


def test_2_the_longest_row(h):
    L = 1 << 20
    ids, off = sc.ragged([5, 70000, 0, 3])
    want = sc.restate_np(ids, off, L, B, E, P, IGN, 0)
    assert want[8] == 1
    check_device(h, ids, off, L, B, E, cap=1, want=want)


# ---- 3. capacity and NULL outputs
@pytest.mark.parametrize("L,bos,eos", [(8, B, E), (5, B, -1), (64, -1, E)])
def test_3_capacity(h, L, bos, eos):
    ids, off = pc.mixed(90, 5 + L, max(L, 8))
    want = sc.restate(ids, off, L, bos, eos, P, IGN, 0)
    R = want[8]
    assert R > 4
    for cap in (0, 1, R - 1, R, R + 3):
        check_device(h, ids, off, L, bos, eos, cap=cap, want=want)      # status bit 0 exactly when R > cap


def test_3_every_subset_of_null_outputs(h):
    """every output but d_nrows_out may be NULL: all 2^8 subsets of the eight arrays, at a capacity that fits and at one that does not"""
    ids, off = pc.mixed(40, 11, 8)
    want = sc.restate(ids, off, 8, B, E, P, IGN, 0)
    for outs in itertools.product((False, True), repeat=8):
        check_device(h, ids, off, 8, B, E, outs=outs, want=want)
        check_device(h, ids, off, 8, B, E, cap=want[8] - 1, outs=outs, want=want)     # the size query reports no drop: nothing was asked for


# ---- 4. alignment
@pytest.mark.parametrize("L", [8, 7])
@pytest.mark.parametrize("shifts", [(0, 0, 0, 0), (1, 0, 0, 0), (0, 2, 0, 0), (0, 0, 3, 0), (0, 0, 0, 1), (1, 2, 3, 1), (3, 3, 3, 3), (2, 1, 0, 3)])
def test_4_alignment(h, L, shifts):
    """each plane `shift` elements behind a 16-byte boundary; the ids one element, the offsets one element into larger buffers"""
    ids, off = pc.mixed(50, 17, 8)
    want = sc.restate(ids, off, L, B, E, P, IGN, 0)
    R, nseq = want[8], len(off) - 1
    ids_buf = torch.full((len(ids) + 9,), 777777, dtype=torch.int32, device="cuda"); ids_buf[1:1 + len(ids)] = torch.from_numpy(ids).cuda()
    off_buf = torch.full((len(off) + 5,), -5, dtype=torch.int64, device="cuda"); off_buf[1:1 + len(off)] = torch.from_numpy(off).cuda()
    bufs = [canary(R * L + 64) for _ in range(4)]
    assert all(b.data_ptr() % 16 == 0 for b in bufs)
    planes = [b[s:] for b, s in zip(bufs, shifts)]
    nrows = torch.zeros(2, dtype=torch.int64, device="cuda")
    assert device_call(h, ids_buf[1:], len(ids), off_buf[1:], nseq, L, B, E, P, IGN, 0, planes + [None, None], R, None, None, nrows) == 0
    assert status(h) == 0 and nrows.tolist() == [R, want[9]]
    for b, s, w in zip(bufs, shifts, want[:4]):
        g = b.cpu().numpy()
        assert np.array_equal(g[s:s + R * L], w.reshape(-1)) and (g[:s] == CANARY).all() and (g[s + R * L:] == CANARY).all(), (L, shifts)


# ---- 5. bad ranges
def test_5_bad_ranges(h):
    ids = (1000 + np.arange(60)).astype(np.int32)
    for off, ids_len in (([0, 5, 3, 12, 20], 60),             # decreasing
                         ([0, 10, 70, 70, 80], 60),            # a range past ids_len
                         ([0, 10, 20, 35, 60], 30),            # ids_len below id_offsets[nseq]: a tokenizer call that overflowed its ids_cap
                         ([-1, 4, 9], 60)):
        off = np.array(off, dtype=np.int64)
        want = check_device(h, ids, off, 8, B, E, ids_len=ids_len)
        assert want[10] == 8
        flat = want[0].reshape(-1)
        for q in range(len(off) - 1):
            at = int(want[6][q]) * 8 + int(want[7][q])
            if off[q] < 0 or off[q + 1] < off[q] or off[q + 1] > ids_len:      # read as empty: its specials only
                assert flat[at:at + 2].tolist() == [B, E]
            else:                                                               # neighbours intact
                k = int(off[q + 1] - off[q])
                assert flat[at:at + k + 2].tolist() == [B] + ids[off[q]:off[q + 1]].tolist() + [E]
    # the host form takes the ids up to the largest offset: decreasing offsets there too
    off = np.array([0, 5, 3, 12, 20], dtype=np.int64)
    want = sc.restate(ids, off, 8, B, E, P, IGN, 0, ids_len=20)
    got = bf.ids_to_stream_rows_batch(h, ids, off, 8, B, E, P)
    assert all(np.array_equal(g, w) for g, w in zip(got, want[:8])) and bf.lib().BfLastStatus(vp(h)) == 8


def test_5_behind_a_tokenizer_call_that_overflowed(h):
    """TextToIdsBatchDevice with an ids_cap too small, the stream call behind it on the same stream with ids_len = that capacity and no
    synchronisation between them: the documents whose ids did not fit contribute their specials only, the others their exact units"""
    docs = [b"hello world again", b"unaffable telescope", b"a b c d e f g h i j k l m n o p", b"the end"]
    text, doff = bf.pack_docs(docs)
    full_ids, full_off = bf.text_to_ids_batch(h, (text, doff), 64, 0)
    cap = int(full_off[2]) + 3                                 # documents 0 and 1 fit, 2 and 3 do not
    d_text = torch.from_numpy(text.copy()).cuda(); d_doff = torch.from_numpy(doff).cuda()
    d_ids = torch.full((cap,), -1, dtype=torch.int32, device="cuda")
    d_ids, d_idoff = bf.text_to_ids_batch_device(h, d_text, d_doff, 64, 0, out_ids=d_ids)
    got = bf.ids_to_stream_rows_batch_device(h, d_ids, d_idoff, 16, None, 50256, 50256, rows_cap=8)
    assert status(h) == 8
    want = sc.restate(full_ids, full_off, 16, -1, 50256, 50256, IGN, 0, ids_len=cap)
    R = want[8]
    assert 0 < R <= 8 and got[8].tolist() == [R, want[9]]
    for g, w in zip(got[:6], want[:6]):
        assert np.array_equal(g.cpu().numpy()[:R], w)
    assert np.array_equal(got[6].cpu().numpy(), want[6]) and np.array_equal(got[7].cpu().numpy(), want[7])
    assert want[9] == int(full_off[2]) + 4 and want[0][0][0] == full_ids[0]      # two documents whole, two ends of text alone


# ---- 6. arguments
def test_6_refused_arguments(h):
    ids = torch.arange(4, dtype=torch.int32, device="cuda"); off = torch.tensor([0, 4], dtype=torch.int64, device="cuda")
    nrows = torch.full((2,), -1, dtype=torch.int64, device="cuda")
    ok = dict(L=8, bos=1, eos=2, pad=0, ign=-100, flags=0)

    def call(hm=h, d_ids=ids, ids_len=4, nseq=1, cap=0, d_off=off, d_nrows=nrows, **kw):
        a = dict(ok, **kw)
        return device_call(hm, d_ids, ids_len, d_off, nseq, a["L"], a["bos"], a["eos"], a["pad"], a["ign"], a["flags"], [None] * 6, cap, None, None, d_nrows)
    assert call() == 0 and status(h) == 0 and nrows.tolist() == [1, 6]
    for bad in (dict(L=0), dict(L=-3), dict(L=(1 << 20) + 1), dict(flags=8), dict(flags=-1), dict(flags=1 << 8)):
        assert call(**bad) == E_ARG, bad
    for fine in (dict(L=1), dict(L=2), dict(L=1 << 20), dict(pad=-7), dict(flags=7), dict(ign=0), dict(L=1, bos=-1, eos=-1)):
        assert call(**fine) == 0, fine                          # no body >= 1 condition: L = 1 with both specials is fine
    assert call(L=1) == 0 and status(h) == 0 and nrows.tolist() == [6, 6]
    assert call(hm=None) == E_ARG                              # a NULL handle
    assert call(nseq=-1) == E_ARG and call(nseq=1 << 31) == E_ARG and call(cap=-1) == E_ARG and call(d_off=None) == E_ARG and call(d_nrows=None) == E_ARG
    assert call(d_ids=None) == E_ARG and call(ids_len=-1) == E_ARG
    assert call(d_ids=None, ids_len=0) == 0 and status(h) == 8      # no ids may be read: the sequence is outside [0, 0]
    # the INT32 bound of the row count, from what the host knows: a claimed ids_len of 2^31 over tiny real arrays
    assert call(L=1, ids_len=1 << 31) == E_ARG and call(L=1, bos=-1, eos=-1, ids_len=(1 << 31) - 1) == 0 and call(L=1, bos=-1, ids_len=(1 << 31) - 1) == E_ARG
    assert call(L=2, ids_len=1 << 31) == 0 and status(h) == 0 and nrows.tolist() == [3, 6]
    hi = np.arange(4, dtype=np.int32); ho = np.array([0, 4], dtype=np.int64)
    f = bf.lib().IdsToStreamRowsBatch
    tail = (None,) * 6 + (0, None, None)
    assert f(vp(h), hi.ctypes.data, ho.ctypes.data, 1, 8, 1, 2, 0, -100, 0, *tail) == 1
    assert f(None, hi.ctypes.data, ho.ctypes.data, 1, 8, 1, 2, 0, -100, 0, *tail) == E_ARG
    assert f(vp(h), hi.ctypes.data, ho.ctypes.data, 1, 0, 1, 2, 0, -100, 0, *tail) == E_ARG
    assert f(vp(h), hi.ctypes.data, ho.ctypes.data, 1, 8, 1, 2, 0, -100, 8, *tail) == E_ARG
    assert f(vp(h), hi.ctypes.data, None, 1, 8, 1, 2, 0, -100, 0, *tail) == E_ARG
    assert f(vp(h), None, ho.ctypes.data, 1, 8, 1, 2, 0, -100, 0, *tail) == E_ARG
    assert f(vp(h), hi.ctypes.data, ho.ctypes.data, -1, 8, 1, 2, 0, -100, 0, *tail) == E_ARG
    assert f(vp(h), hi.ctypes.data, ho.ctypes.data, 1, 8, 1, 2, 0, -100, 0, *(None,) * 6, -1, None, None) == E_ARG
    neg = np.array([-1, 3], dtype=np.int64)                    # the host form reads ids from id_offsets[0] on: a negative one is refused
    assert f(vp(h), hi.ctypes.data, neg.ctypes.data, 1, 8, 1, 2, 0, -100, 0, *tail) == E_ARG


def test_6_no_sequences(h):
    off = torch.zeros(1, dtype=torch.int64, device="cuda")
    check_device(h, np.zeros(0, dtype=np.int32), np.zeros(1, dtype=np.int64), 8, B, E, cap=4)      # R = 0: nothing is written
    nrows = torch.full((2,), -1, dtype=torch.int64, device="cuda")
    assert device_call(h, None, 0, off, 0, 8, B, E, P, IGN, 0, [None] * 6, 0, None, None, nrows) == 0 and status(h) == 0 and nrows.tolist() == [0, 0]
    got = bf.ids_to_stream_rows_batch(h, np.zeros(0, dtype=np.int32), np.zeros(1, dtype=np.int64), 8, B, E)
    assert [g.shape for g in got] == [(0, 8)] * 4 + [(0,)] * 4


def test_6_handles_of_every_kind():
    import w2h_cases
    ids, off = pc.synthetic(6)
    kinds = []
    for path in (bfutil.model_path(bfutil.bert_model_name()), bfutil.model_path("gpt2.bin"), bfutil.model_path("bert_base_tok.i2w"), w2h_cases.FIXTURE):
        hm = bf.load_model(path)
        try:
            kinds.append(bf.lib().BfModelKind(vp(hm)))
            assert bf.lib().BfReserve(vp(hm), 64, 1 << 12, 0) == 0      # every kind: the workspaces of this call too
            grows0 = bf.workspace_grows()
            check_device(hm, ids, off, 8, B, E)
            assert bf.workspace_grows() == grows0
            check_host(hm, ids, off, 8, B, E)
        finally:
            bf.free_model(hm)
    assert kinds == [0, 3, 5, 6]                               # WordPiece, BPE, [i2w] only, [w2h] only


# ---- 7. the host form
def test_7_host_form(h):
    L = 8
    ids, off = pc.mixed(70, 23, L)
    ids = np.ascontiguousarray(ids, dtype=np.int32); off = np.ascontiguousarray(off, dtype=np.int64)
    want = sc.restate(ids, off, L, B, E, P, IGN, 0)
    R, nseq = want[8], len(off) - 1
    f = bf.lib().IdsToStreamRowsBatch
    pre = (vp(h), ids.ctypes.data, off.ctypes.data, nseq, L, B, E, P, IGN, 0)
    # the size query needs no capacity, with and without the per-sequence outputs
    assert f(*pre, *(None,) * 6, 0, None, None) == R
    seq = [np.full(nseq, CANARY, dtype=np.int32) for _ in range(2)]
    assert f(*pre, *(None,) * 6, 0, seq[0].ctypes.data, seq[1].ctypes.data) == R
    assert np.array_equal(seq[0], want[6]) and np.array_equal(seq[1], want[7])
    # BF_E_CAPACITY: the sequence outputs complete, nothing else written
    for cap in (0, R - 1):
        outs = [np.full((cap, L), CANARY, dtype=np.int32) for _ in range(4)] + [np.full(cap + 1, CANARY, dtype=np.int32) for _ in range(2)]
        seq = [np.full(nseq, CANARY, dtype=np.int32) for _ in range(2)]
        assert f(*pre, *[o.ctypes.data for o in outs], cap, seq[0].ctypes.data, seq[1].ctypes.data) == E_CAPACITY
        assert all((o == CANARY).all() for o in outs)
        assert np.array_equal(seq[0], want[6]) and np.array_equal(seq[1], want[7])
    # each row output alone in buffers larger than needed: what was asked for equals the restatement, nothing else is touched
    for k in range(6):
        outs = [np.full((R + 2, L), CANARY, dtype=np.int32) for _ in range(4)] + [np.full(R + 2, CANARY, dtype=np.int32) for _ in range(2)]
        assert f(*pre, *[o.ctypes.data if i == k else None for i, o in enumerate(outs)], R + 2, None, None) == R
        for i, o in enumerate(outs):
            n = R if i == k else 0
            assert np.array_equal(o[:n], want[i][:n]) and (o[n:] == CANARY).all(), (k, i)


# ---- 8. end to end
@pytest.fixture(scope="module")
def fx():
    return rc.load_fixture()


CLM_MODELS = {"gpt2.bin": dict(bos=None, eos=50256, pad=50256, unk=0), "bert_base_tok.bin": dict(bos=101, eos=102, pad=0, unk=100)}


@pytest.mark.parametrize("model", sorted(CLM_MODELS))
@pytest.mark.parametrize("L,drop_last", [(64, False), (64, True), (7, False)])
def test_8_text_to_stream_rows(fx, model, L, drop_last):
    sp = CLM_MODELS[model]
    docs = rc.encode_docs()
    ref_ids, ref_off = rc.fixture_ids(fx, model, rc.INT32_MAX)       # the stored reference ids, untruncated
    bos = -1 if sp["bos"] is None else sp["bos"]
    want = sc.restate_np(ref_ids, ref_off, L, bos, sp["eos"], sp["pad"], IGN, 1 if drop_last else 0)
    R, T = want[8], want[9]
    if model == "gpt2.bin" and L == 64:
        assert T == 4556 and R == (71 if drop_last else 72)
    hm = bf.load_model(bfutil.model_path(model))
    try:
        text, off = bf.pack_docs(docs)
        d_text = torch.from_numpy(text.copy()).cuda(); d_off = torch.from_numpy(off).cuda()
        for got in (bf.encode_clm_batch(hm, docs, L, sp["bos"], sp["eos"], sp["pad"], sp["unk"], drop_last=drop_last),
                    bf.encode_clm_batch_device(hm, d_text, d_off, L, sp["bos"], sp["eos"], sp["pad"], sp["unk"], drop_last=drop_last, rows_cap=R + 1)):
            torch.cuda.synchronize()
            assert list(got) == ["input_ids", "seg", "pos", "labels", "row_first_seq", "row_first_pos", "seq_row", "seq_col", "nrows"]
            assert all(got[k].dtype == torch.int32 for k in list(got)[:8]) and got["nrows"].dtype == torch.int64 and got["nrows"].tolist() == [R, T]
            assert got["input_ids"].shape[0] >= R and got["input_ids"].shape[1] == L and got["seq_row"].shape == (len(docs),)
            for k, w in zip(list(got)[:6], want[:6]):
                assert np.array_equal(got[k].cpu().numpy()[:R], w), k
            assert np.array_equal(got["seq_row"].cpu().numpy(), want[6]) and np.array_equal(got["seq_col"].cpu().numpy(), want[7])
            assert bf.lib().BfLastStatus(vp(hm)) == 0
    finally:
        bf.free_model(hm)


def test_8_repeated_call_after_reserve_allocates_nothing():
    """BfWorkspaceGrows is unchanged across the first and a repeated encode_clm_batch_device on a reserved handle; the two give identical tensors"""
    docs = rc.encode_docs() * 8
    text, off = bf.pack_docs(docs)
    hm = bf.load_model(bfutil.model_path("gpt2.bin"))
    try:
        bf.reserve(hm, len(docs), len(text))
        grows0 = bf.workspace_grows()
        d_text = torch.from_numpy(text.copy()).cuda(); d_off = torch.from_numpy(off).cuda()
        a = bf.encode_clm_batch_device(hm, d_text, d_off, 64, None, 50256, 50256)
        torch.cuda.synchronize()
        assert bf.workspace_grows() == grows0, "the FIRST call on the reserved handle made the library allocate device memory (BfWorkspaceGrows)"
        R, T = a["nrows"].tolist()
        assert R == -(-T // 64) and 0 < R <= a["input_ids"].shape[0]
        b = bf.encode_clm_batch_device(hm, d_text, d_off, 64, None, 50256, 50256)
        torch.cuda.synchronize()
        assert bf.workspace_grows() == grows0, "the repeated call made the library allocate device memory (BfWorkspaceGrows)"
        for k in a:
            n = R if k in ("input_ids", "seg", "pos", "labels", "row_first_seq", "row_first_pos") else len(a[k])
            assert np.array_equal(a[k].cpu().numpy()[:n], b[k].cpu().numpy()[:n]), k
    finally:
        bf.free_model(hm)


# ---- 9. the MLM call over stream rows
def test_9_mlm_over_stream_rows(h):
    """RowsMlmMaskBatchDevice with d_nrows = the first entry of the call's d_nrows_out and d_seg = its segment plane processes exactly R rows"""
    ids, off = pc.mixed(60, 3, 8)
    want = sc.restate(ids, off, 8, B, E, P, IGN, 0)
    R = want[8]
    got = bf.ids_to_stream_rows_batch_device(h, torch.from_numpy(ids).cuda(), torch.from_numpy(off).cuda(), 8, B, E, P, rows_cap=R + 2)
    assert got[8].tolist() == [R, want[9]] and got[0].shape == (R + 2, 8)
    rows, seg = got[0], got[1]
    rows[R:] = 4242; seg[R:] = 1                              # what lies behind R rows is the caller's: eligible cells, if the call looked at them
    mids, mlabels = bf.rows_mlm_mask_device(h, rows, seg=seg, nrows=got[8][:1], special_ids=(B, E), select_prob=1.0, mask_prob=1.0, random_prob=0.0, mask_id=7,
                                            rand_range=(1000, 2000), seed=5)
    torch.cuda.synchronize()
    rows, seg, mids, mlabels = (t.cpu().numpy() for t in (rows, seg, mids, mlabels))
    assert (mlabels[R:] == IGN).all() and (mids[R:] == 4242).all()
    elig = (seg[:R] != 0) & (rows[:R] != B) & (rows[:R] != E)
    assert elig.sum() == len(ids) and (mids[:R][elig] == 7).all() and np.array_equal(mlabels[:R][elig], rows[:R][elig]) and (mlabels[:R][~elig] == IGN).all()
