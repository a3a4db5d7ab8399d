"""GPU: IdsToPairRowsBatchDevice / IdsToPairRowsBatch (bf_kernels_pairs.hip) and the Python calls above them against the numpy restatement of
the specification (pair_cases.restate): the parameter table on synthetic pairs, the capacity guard over canary-filled buffers, unaligned
outputs and inputs inside larger buffers, pair counts around the scan tile with neighbours of different geometry, one pair of very many
windows, bad ranges on either side, refused arguments, handles of every kind, and two texts -> rows end to end against the stored
reference ids of the rows stage (tests/golden/rows/encode_ids.json)."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import bfutil
import blingfire_amd as bf
import pair_cases as pc
import rows_cases as rc

pytestmark = pytest.mark.gpu

CANARY32, CANARY8 = -0x35014542, 0xA5
CANARIES = (CANARY32, CANARY8, CANARY8, CANARY32, CANARY32)
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
    return None if t is None else t if isinstance(t, int) else t.data_ptr()


def spec_args(par, pad_id=pc.PAD):
    L, cls_id, sep_id, double_sep, mode, max_a, stride, max_rows, pad_left = par
    return (L, cls_id, sep_id, pad_id, mode, max_a, stride, max_rows, pc.flags(pad_left, double_sep))


def device_call(hm, ids_a, len_a, off_a, ids_b, len_b, off_b, nseq, par, outs, cap, r_off):
    """ids / offsets / outputs: tensors, raw addresses or None"""
    return bf.lib().IdsToPairRowsBatchDevice(vp(hm), ptr(ids_a), len_a, ptr(off_a), ptr(ids_b), len_b, ptr(off_b), nseq, *spec_args(par),
                                             *[ptr(o) for o in outs], cap, ptr(r_off), None)


def host_call(hm, src, par, outs, cap, r_off):
    a = [np.ascontiguousarray(x, dtype=t) for x, t in zip(src, (np.int32, np.int64, np.int32, np.int64))]
    return bf.lib().IdsToPairRowsBatch(vp(hm), a[0].ctypes.data, a[1].ctypes.data, a[2].ctypes.data, a[3].ctypes.data, len(a[1]) - 1, *spec_args(par),
                                       *[None if o is None else o.ctypes.data for o in outs], cap, None if r_off is None else r_off.ctypes.data)


def restate(src, par, **kw):
    L, cls_id, sep_id, double_sep, mode, max_a, stride, max_rows, pad_left = par
    return pc.restate(*src, L, cls_id, sep_id, pc.PAD, mode, max_a, stride, max_rows, pad_left, double_sep, **kw)


def canaries(cap, L, tail=0):
    """canary-filled outputs of cap rows (+ tail elements the call must not touch either): rows, mask, type, pair, first B id"""
    return [torch.full((cap * L + tail,), CANARY32, dtype=torch.int32, device="cuda"), torch.full((cap * L + tail,), CANARY8, dtype=torch.uint8, device="cuda"),
            torch.full((cap * L + tail,), CANARY8, dtype=torch.uint8, device="cuda"), torch.full((cap + tail,), CANARY32, dtype=torch.int32, device="cuda"),
            torch.full((cap + tail,), CANARY32, dtype=torch.int32, device="cuda")]


def upload(src):
    return [torch.from_numpy(np.ascontiguousarray(x, dtype=t)).cuda() for x, t in zip(src, (np.int32, np.int64, np.int32, np.int64))]


def check_device(hm, src, par, cap=None, len_a=None, len_b=None, outs=(True,) * 5, want=None, d_src=None):
    """one device call over canary-filled buffers of `cap` rows (default: the total): everything below min(cap, total) equals the
    restatement, nothing at or past it changed, the offsets are complete, the status word is what the restatement says"""
    L = par[0]
    if want is None:
        want = restate(src, par, len_a=len_a, len_b=len_b)
    total = len(want[3])
    cap = total if cap is None else cap
    d = upload(src) if d_src is None else d_src
    bufs = canaries(cap, L, tail=64)
    r_off = torch.full((len(src[1]),), -1, dtype=torch.int64, device="cuda")
    use = [b if u else None for b, u in zip(bufs, outs)]
    r = device_call(hm, d[0], len(src[0]) if len_a is None else len_a, d[1], d[2], len(src[2]) if len_b is None else len_b, d[3], len(src[1]) - 1, par, use, cap, r_off)
    assert r == 0, (par, r)
    st = status(hm)
    k = min(cap, total)
    assert np.array_equal(r_off.cpu().numpy(), want[5]), par
    for i, (b, w, width, can) in enumerate(zip(bufs, want[:5], (L, L, L, 1, 1), CANARIES)):
        g = b.cpu().numpy()
        if outs[i]:
            assert np.array_equal(g[:k * width], w[:k].reshape(-1)), (par, cap, i)
            assert (g[k * width:] == can).all(), (par, cap, i)
        else:
            assert (g == can).all(), (par, cap, i)
    dropped = 1 if (total > cap and any(outs)) else 0
    assert st == want[6] | dropped, (par, cap, st)
    return want


def check_host(hm, src, par, want=None):
    L, cls_id, sep_id, double_sep, mode, max_a, stride, max_rows, pad_left = par
    if want is None:
        want = restate(src, par)
    got = bf.ids_to_pair_rows_batch(hm, *src, L, cls_id, sep_id, pc.PAD, mode, max_a, stride, max_rows, pad_left, double_sep)
    for g, w in zip(got, want[:6]):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), par


# ---- 1. the parameter table on synthetic pairs
@pytest.mark.parametrize("L", pc.TABLE_L)
def test_1_parameter_table(h, L):
    n = 0
    for par in pc.table():
        if par[0] != L:
            continue
        src = pc.synthetic(par, seed=n)
        want = check_device(h, src, par)
        check_host(h, src, par, want)
        n += 1
    assert n > 0


# ---- 2. capacity
CAPACITY_PARS = [(8, pc.CLS, pc.SEP, False, 0, 2, 1, 0, False), (63, pc.CLS, -1, False, 0, 1, 1, 3, True), (64, pc.CLS, pc.SEP, True, 0, 59, 0, 0, False),
                 (64, pc.CLS, pc.SEP, False, 1, 0, 0, 1, False)]


@pytest.mark.parametrize("par", CAPACITY_PARS)
def test_2_capacity(h, par):
    L = par[0]
    src = pc.synthetic(par)
    d_src = upload(src)
    want = restate(src, par)
    total = len(want[3])
    for cap in (0, total - 1, total, total + 1):
        check_device(h, src, par, cap=cap, want=want, d_src=d_src)          # status bit 0 exactly when total > cap
    # the size query: every output NULL (no drop is reported: nothing was asked for), then each optional output NULL in turn
    check_device(h, src, par, cap=0, outs=(False,) * 5, want=want, d_src=d_src)
    for drop in range(5):
        check_device(h, src, par, outs=tuple(i != drop for i in range(5)), want=want, d_src=d_src)
        check_device(h, src, par, cap=total - 1, outs=tuple(i != drop for i in range(5)), want=want, d_src=d_src)
    # host form: BF_E_CAPACITY, offsets complete, nothing else written
    for cap in (0, total - 1):
        outs = [np.full((cap, L), CANARY32, dtype=np.int32), np.full((cap, L), CANARY8, dtype=np.uint8), np.full((cap, L), CANARY8, dtype=np.uint8),
                np.full(cap, CANARY32, dtype=np.int32), np.full(cap, CANARY32, dtype=np.int32)]
        r_off = np.full(len(src[1]), -1, dtype=np.int64)
        assert host_call(h, src, par, outs, cap, r_off) == E_CAPACITY and np.array_equal(r_off, want[5])
        assert all((o == c).all() for o, c in zip(outs, CANARIES))
    r_off = np.full(len(src[1]), -1, dtype=np.int64)
    assert host_call(h, src, par, [None] * 5, 0, r_off) == total and np.array_equal(r_off, want[5])       # the size query needs no capacity
    for keep in range(5):                                                                                   # one output alone
        outs = [np.full((total, L), CANARY32, dtype=np.int32), np.full((total, L), CANARY8, dtype=np.uint8), np.full((total, L), CANARY8, dtype=np.uint8),
                np.full(total, CANARY32, dtype=np.int32), np.full(total, CANARY32, dtype=np.int32)]
        assert host_call(h, src, par, [o if i == keep else None for i, o in enumerate(outs)], total, r_off) == total
        assert all(np.array_equal(o, want[i]) if i == keep else (o == CANARIES[i]).all() for i, o in enumerate(outs))


# ---- 3. alignment
@pytest.mark.parametrize("L", [64, 63])
def test_3_alignment(h, L):
    """rows, mask and type each 0, 1, 2 or 4 elements behind a 16-byte boundary, independently; ids and offsets of both sides at odd element
    addresses inside larger buffers: the rows are exact, nothing around the outputs and nothing of the inputs' buffers changed"""
    import pointer_cases as pt
    par = (L, pc.CLS, pc.SEP, False, 0, 7, 3, 0, False)
    src = pc.synthetic(par)
    want = restate(src, par)
    total = len(want[3])
    nseq = len(src[1]) - 1
    placed = [pt.place(np.ascontiguousarray(x), shift, b"\xff", b"\xff") for x, shift in zip(src, (4, 8, 12, 24))]
    r_off = torch.empty(nseq + 1, dtype=torch.int64, device="cuda")
    for sr, sm, st in itertools.product((0, 1, 2, 4), repeat=3):
        rooms = [pt.room(np.int32, total * L, sr), pt.room(np.uint8, total * L, sm), pt.room(np.uint8, total * L, st)]
        r = device_call(h, placed[0].addr, len(src[0]), placed[1].addr, placed[2].addr, len(src[2]), placed[3].addr, nseq, par,
                        [rooms[0].addr, rooms[1].addr, rooms[2].addr, None, None], total, r_off)
        assert r == 0 and status(h) == 0
        for room, w in zip(rooms, want[:3]):
            assert np.array_equal(room.fetch().result(), w.reshape(-1)), (sr, sm, st)
            room.untouched(total * L, "shifts %d %d %d" % (sr, sm, st))
    assert np.array_equal(r_off.cpu().numpy(), want[5])
    for p in placed:
        p.verify("pair inputs")


# ---- 4. scale and geometry
def alternating(nseq, seed, max_a, longest=24):
    """neighbouring pairs alternate na = 0 and na = max_a: their body_b and step differ, so a row that takes its neighbour's shows"""
    rnd = np.random.RandomState(seed)
    la = [0 if q % 2 == 0 else max_a for q in range(nseq)]
    lb = rnd.randint(0, longest, size=nseq)
    lb[rnd.randint(0, nseq, size=max(1, nseq // 50))] = 0
    return pc.ragged(la, pc.A0) + pc.ragged(lb, pc.B0)


@pytest.mark.parametrize("nseq", [1, 1023, 1024, 1025, 5000])
def test_4_pair_counts_around_the_scan_tile(h, nseq):
    src = alternating(nseq, nseq, 2)
    d_src = upload(src)
    want = check_device(h, src, (8, pc.CLS, pc.SEP, False, 0, 2, 1, 0, False), d_src=d_src)
    same = want[3][1:] == want[3][:-1]                                      # (the table itself: neighbours do step differently)
    steps = set(zip((want[3][1:][same] % 2).tolist(), np.diff(want[4])[same].tolist()))
    assert steps <= {(0, 4), (1, 2)} and (nseq < 1000 or steps == {(0, 4), (1, 2)})
    check_host(h, src, (8, pc.CLS, pc.SEP, False, 0, 2, 1, 0, False), want)
    check_device(h, src, (12, pc.CLS, pc.SEP, True, 0, 2, 0, 2, True), d_src=d_src)
    check_device(h, src, (12, pc.CLS, pc.SEP, False, 1, 0, 0, 1, False), d_src=d_src)


def test_4_one_pair_of_very_many_windows(h):
    """B of 200,000 ids at L = 8 (T = 5, ka = 2, stride 1: 100,000 windows two ids apart) among short pairs; also with neither the pair nor the
    first B id of a row taken, where the fill has workspace for the first rows only and finds the rest by its own search"""
    la = [3, 0, 2, 2, 1, 0, 5]
    lb = [3, 0, 7, 200000, 1, 6, 9]
    src = pc.ragged(la, pc.A0) + pc.ragged(lb, pc.B0)
    d_src = upload(src)
    par = (8, pc.CLS, pc.SEP, False, 0, 2, 1, 0, False)
    want = check_device(h, src, par, d_src=d_src)
    assert want[5][4] - want[5][3] == 1 + (200000 - 3 + 1) // 2 and want[4][want[5][4] - 1] == 2 * (want[5][4] - want[5][3] - 1)
    check_device(h, src, par, outs=(True, True, True, False, False), want=want, d_src=d_src)
    check_device(h, src, (8, -1, -1, False, 0, 0, 0, 0, True), outs=(True, False, True, False, True), d_src=d_src)


# ---- 5. bad ranges, shared arrays, chaining, arguments, handles
BAD = [([0, 5, 3, 12, 20], 60), ([0, 10, 70, 70, 80], 60), ([0, 10, 20, 35, 60], 30), ([-1, 4, 9, 12, 13], 60)]
GOOD = ([0, 3, 9, 9, 30], 60)


@pytest.mark.parametrize("par", [(8, pc.CLS, pc.SEP, False, 0, 2, 1, 0, False), (9, pc.CLS, pc.SEP, True, 1, 0, 0, 1, True)])
def test_5_bad_ranges(h, par):
    ids_a = (pc.A0 + np.arange(60)).astype(np.int32); ids_b = (pc.B0 + np.arange(60)).astype(np.int32)
    for (oa, la), (ob, lb) in [(b, GOOD) for b in BAD] + [(GOOD, b) for b in BAD] + [(BAD[0], BAD[1]), (BAD[2], BAD[3])]:
        want = check_device(h, (ids_a, oa, ids_b, ob), par, len_a=la, len_b=lb)
        assert want[6] == 8
    # the host form takes each side's ids up to its largest offset: decreasing offsets there too
    src = (ids_a, BAD[0][0], ids_b, GOOD[0])
    want = restate(src, par, len_a=20, len_b=30)
    check_host(h, src, par, want)
    assert bf.lib().BfLastStatus(vp(h)) == 8


def test_5_both_sides_in_one_array(h):
    """ids_a and ids_b the same device array: A the sequences as they are, B the same sequences in reverse order"""
    ids, off = pc.ragged([3, 0, 9, 4, 17, 1], pc.A0)
    d_ids = torch.from_numpy(ids).cuda()
    rev_off = np.array([int(off[5 - q]) for q in range(6)] + [int(off[1])], dtype=np.int64)       # decreasing: B of every pair but the last is a bad range
    pair_off = np.concatenate([off[3:], off[-1:].repeat(3)])                                      # B = sequences 3, 4, 5, then three empty ones
    for ob, bit in ((off, 0), (pair_off, 0), (rev_off, 8)):
        par = (10, pc.CLS, pc.SEP, False, 0, 3, 1, 0, False)
        want = restate((ids, off, ids, ob), par)
        assert want[6] == bit
        d = [d_ids, torch.from_numpy(off).cuda(), d_ids, torch.from_numpy(np.ascontiguousarray(ob)).cuda()]
        check_device(h, (ids, off, ids, ob), par, want=want, d_src=d)


def test_5_behind_a_tokenizer_call_that_overflowed(h):
    """two TextToIdsBatchDevice calls, the second with an ids_cap too small, IdsToPairRowsBatchDevice behind them on the same stream with
    ids_b_len = that capacity, no synchronisation between them: the pairs whose B did not fit have an empty B, the others their exact rows"""
    docs_a = [b"first question", b"second one here", b"third", b"the fourth question is long enough to be cut"]
    docs_b = [b"hello world again", b"unaffable telescope", b"a b c d e f g h i j k l m n o p", b"the end"]
    ta, oa = bf.pack_docs(docs_a); tb, ob = bf.pack_docs(docs_b)
    full_a, foff_a = bf.text_to_ids_batch(h, (ta, oa), 64, 100)
    full_b, foff_b = bf.text_to_ids_batch(h, (tb, ob), 64, 100)
    cap = int(foff_b[2]) + 3                                   # B of pairs 0 and 1 fits, of 2 and 3 does not
    d_ids_a, d_off_a = bf.text_to_ids_batch_device(h, torch.from_numpy(ta.copy()).cuda(), torch.from_numpy(oa).cuda(), 64, 100)
    d_ids_b = torch.full((cap,), -1, dtype=torch.int32, device="cuda")
    d_ids_b, d_off_b = bf.text_to_ids_batch_device(h, torch.from_numpy(tb.copy()).cuda(), torch.from_numpy(ob).cuda(), 64, 100, out_ids=d_ids_b)
    got = bf.ids_to_pair_rows_batch_device(h, d_ids_a, d_off_a, d_ids_b, d_off_b, 16, pc.CLS, pc.SEP, pc.PAD, mode=0, max_a=4, stride=2, max_rows_per_pair=0)
    assert status(h) == 8
    assert np.array_equal(d_off_b.cpu().numpy(), foff_b)
    want = pc.restate(full_a, foff_a, full_b, foff_b, 16, pc.CLS, pc.SEP, pc.PAD, 0, 4, 2, 0, len_b=cap)
    for g, w in zip(got, want[:6]):
        assert np.array_equal(g.cpu().numpy(), w)
    r2, ka = int(want[5][2]), min(int(foff_a[3] - foff_a[2]), 4)
    assert want[5][3] == r2 + 1 and want[0][0][1] == full_a[0]
    assert want[0][r2].tolist() == [pc.CLS] + full_a[foff_a[2]:foff_a[2] + ka].tolist() + [pc.SEP, pc.SEP] + [pc.PAD] * (13 - ka)


def test_5_refused_arguments(h):
    ids = torch.arange(4, dtype=torch.int32, device="cuda"); off = torch.tensor([0, 4], dtype=torch.int64, device="cuda")
    r_off = torch.full((2,), -1, dtype=torch.int64, device="cuda")
    ok = dict(L=8, cls_id=1, sep_id=2, double_sep=False, mode=0, max_a=2, stride=1, max_rows=0, pad_left=False)

    def call(hm=h, len_a=4, len_b=4, nseq=1, cap=0, d_off_a=off, d_off_b=off, d_r_off=r_off, flags=None, **kw):
        a = dict(ok, **kw)
        par = tuple(a[k] for k in ("L", "cls_id", "sep_id", "double_sep", "mode", "max_a", "stride", "max_rows", "pad_left"))
        if flags is None:
            return device_call(hm, ids, len_a, d_off_a, ids, len_b, d_off_b, nseq, par, [None] * 5, cap, d_r_off)
        return bf.lib().IdsToPairRowsBatchDevice(vp(hm), ptr(ids), 4, ptr(off), ptr(ids), 4, ptr(off), 1, 8, 1, 2, 0, 0, 2, 1, 0, flags, None, None, None, None, None, 0,
                                                 ptr(r_off), None)
    assert call() == 0 and call(mode=1, max_a=0, stride=0, max_rows=1) == 0
    for bad in (dict(L=0), dict(L=-3), dict(L=(1 << 20) + 1), dict(L=3), dict(L=4, double_sep=True), dict(L=1, sep_id=-1), dict(mode=2), dict(mode=-1),
                dict(max_a=-1), dict(max_a=5), dict(stride=-1), dict(stride=3), dict(max_a=4, stride=1), dict(max_rows=-1), dict(sep_id=-1, double_sep=True),
                dict(mode=1), dict(mode=1, max_a=1, stride=0, max_rows=1), dict(mode=1, max_a=0, stride=1, max_rows=1), dict(mode=1, max_a=0, stride=0, max_rows=0),
                dict(mode=1, max_a=0, stride=0, max_rows=2), dict(flags=4), dict(flags=7), dict(flags=1 << 8), dict(flags=-4)):
        assert call(**bad) == E_ARG, bad
    assert call(L=1, cls_id=-1, sep_id=-1, max_a=0, stride=0) == 0 and call(L=1 << 20) == 0 and call(max_a=4, stride=0) == 0 and call(flags=3) == 0
    assert call(hm=None) == E_ARG                              # a NULL handle
    assert call(nseq=-1) == E_ARG and call(len_a=-1) == E_ARG and call(len_b=-1) == E_ARG and call(cap=-1) == E_ARG
    assert call(d_off_a=None) == E_ARG and call(d_off_b=None) == E_ARG and call(d_r_off=None) == E_ARG
    hi = np.arange(4, dtype=np.int32); ho = np.array([0, 4], dtype=np.int64); hr = np.zeros(2, dtype=np.int64); neg = np.array([-1, 3], dtype=np.int64)
    par = (8, 1, 2, False, 0, 2, 1, 0, False)
    assert host_call(h, (hi, ho, hi, ho), par, [None] * 5, 0, hr) == 2
    assert host_call(None, (hi, ho, hi, ho), par, [None] * 5, 0, hr) == E_ARG
    assert host_call(h, (hi, ho, hi, ho), (3,) + par[1:], [None] * 5, 0, hr) == E_ARG
    assert host_call(h, (hi, ho, hi, ho), par, [None] * 5, 0, None) == E_ARG
    assert host_call(h, (hi, neg, hi, ho), par, [None] * 5, 0, hr) == E_ARG      # the host form reads each side from its first offset on: a negative one is refused
    assert host_call(h, (hi, ho, hi, neg), par, [None] * 5, 0, hr) == E_ARG


def test_5_no_pairs(h):
    off = torch.zeros(1, dtype=torch.int64, device="cuda"); r_off = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    bufs = canaries(4, 8)
    assert device_call(h, None, 0, off, None, 0, off, 0, (8, pc.CLS, pc.SEP, False, 1, 0, 0, 1, False), bufs, 4, r_off) == 0
    assert status(h) == 0 and r_off.cpu().tolist() == [0]
    assert all((b.cpu().numpy() == c).all() for b, c in zip(bufs, CANARIES))
    z32, z64 = np.zeros(0, dtype=np.int32), np.zeros(1, dtype=np.int64)
    got = bf.ids_to_pair_rows_batch(h, z32, z64, z32, z64, 8, pc.CLS, pc.SEP)
    assert [g.shape for g in got] == [(0, 8), (0, 8), (0, 8), (0,), (0,), (1,)] and got[5].tolist() == [0]


def test_5_handles_of_every_kind():
    import w2h_cases
    par = (8, pc.CLS, pc.SEP, False, 0, 2, 1, 0, False)
    src = pc.synthetic(par)
    want = restate(src, par)
    kinds = []
    for path in (bfutil.model_path(bfutil.bert_model_name()), bfutil.model_path("gpt2.bin"), bfutil.model_path("bert_base_tok.i2w"), w2h_cases.FIXTURE):
        hm = bf.load_model(path)
        try:
            kinds.append(bf.lib().BfModelKind(vp(hm)))
            assert bf.lib().BfReserve(vp(hm), 64, 1 << 12, 0) == 0      # every kind: the rows workspaces at least
            check_device(hm, src, par, want=want)
            check_host(hm, src, par, want)
        finally:
            bf.free_model(hm)
    assert kinds == [0, 3, 5, 6]                               # WordPiece, BPE, [i2w] only, [w2h] only


# ---- 6. end to end
@pytest.fixture(scope="module")
def fx():
    return rc.load_fixture()


def pair_docs():
    docs = rc.encode_docs()
    return docs, [docs[pc.pair_partner(i, len(docs))] for i in range(len(docs))]


@pytest.mark.parametrize("model", sorted(pc.ENCODE_MODELS))
@pytest.mark.parametrize("case", pc.ENCODE_CASES)
def test_6_texts_to_pair_rows(fx, model, case):
    L, mode, max_a, stride, max_rows, pad_left = case
    sp = pc.ENCODE_MODELS[model]
    len_a, len_b = pc.encode_max_lens(L, mode, max_a, stride, max_rows)
    assert str(len_a) in fx["models"][model] and str(len_b) in fx["models"][model]
    want = pc.restate(*pc.fixture_pairs(fx, model, len_a, len_b), L, sp["cls_id"], sp["sep_id"], sp["pad_id"], mode, max_a, stride, max_rows, pad_left)
    docs_a, docs_b = pair_docs()
    hm = bf.load_model(bfutil.model_path(model))
    try:
        d = []
        for docs in (docs_a, docs_b):
            text, off = bf.pack_docs(docs)
            d += [torch.from_numpy(text.copy()).cuda(), torch.from_numpy(off).cuda()]
        args = (L, sp["cls_id"], sp["sep_id"], sp["pad_id"], sp["unk"], mode, max_a, stride, max_rows, pad_left)
        for got in (bf.encode_pairs_batch(hm, docs_a, docs_b, *args), bf.encode_pairs_batch_device(hm, *d, *args)):
            torch.cuda.synchronize()
            assert [g.dtype for g in got] == [torch.int32, torch.uint8, torch.uint8, torch.int32, torch.int32, torch.int64]
            for g, w in zip(got, want[:6]):
                assert tuple(g.shape) == w.shape and np.array_equal(g.cpu().numpy(), w)
            assert bf.lib().BfLastStatus(vp(hm)) == 0
    finally:
        bf.free_model(hm)


# ---- 7. no allocation after BfReserve
def test_7_repeated_call_after_reserve_allocates_nothing():
    """after BfReserve a repeated encode_pairs_batch_device leaves the device's free memory where it was (hipMemGetInfo): torch serves the
    outputs from its cache, the library's workspaces do not grow"""
    docs_a, docs_b = pair_docs()
    ta, oa = bf.pack_docs(docs_a * 8); tb, ob = bf.pack_docs(docs_b * 8)
    sp = pc.ENCODE_MODELS["bert_base_tok.bin"]
    hm = bf.load_model(bfutil.model_path("bert_base_tok.bin"))
    try:
        bf.reserve(hm, len(oa) - 1, max(len(ta), len(tb)))
        grows0 = bf.workspace_grows()
        d = [torch.from_numpy(x.copy()).cuda() for x in (ta, oa, tb, ob)]
        a = bf.encode_pairs_batch_device(hm, *d, 32, sp["cls_id"], sp["sep_id"], sp["pad_id"], sp["unk"])
        torch.cuda.synchronize()
        assert bf.workspace_grows() == grows0, "the FIRST call on the reserved handle made the library allocate device memory (BfWorkspaceGrows)"
        a = [t.cpu().numpy() for t in a]
        free0 = torch.cuda.mem_get_info()[0]
        b = bf.encode_pairs_batch_device(hm, *d, 32, sp["cls_id"], sp["sep_id"], sp["pad_id"], sp["unk"])
        torch.cuda.synchronize()
        free1 = torch.cuda.mem_get_info()[0]
        assert free1 == free0, "the device's free memory moved by %d bytes across a reserved call" % (free0 - free1)
        assert bf.workspace_grows() == grows0, "the repeated call made the library allocate device memory (BfWorkspaceGrows)"
        for x, y in zip(a, b):
            assert np.array_equal(x, y.cpu().numpy())
        assert a[2].max() == 1 and (a[1].sum(axis=1) >= 3).all()
    finally:
        bf.free_model(hm)
