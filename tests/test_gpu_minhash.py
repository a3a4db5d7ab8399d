"""GPU: IdsToMinHashBatchDevice / IdsToMinHashBatch / MinHashPairsBatchDevice (bf_kernels_minhash.hip) and the Python calls above them against the
sequential restatement of the specification (minhash_cases.restate), by exact equality over canary-filled buffers."""
import ctypes

import numpy as np
import pytest
import torch

import bfutil
import blingfire_amd as bf
import minhash_cases as mc
import rows_cases as rc

pytestmark = pytest.mark.gpu
CANARY = 0x5A
vp = ctypes.c_void_p


@pytest.fixture(scope="module")
def h():
    hm = bf.load_model(bfutil.model_path("bert_base_tok.i2w"))
    yield hm
    bf.free_model(hm)


def status(hm):
    torch.cuda.synchronize()
    return bf.lib().BfLastStatus(vp(hm))


def device_call(hm, ids_, off_, k, H, r, seed, outs, sig_cap, **kw):
    d_ids, d_off = (torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (ids_, off_))
    a = dict(ids=d_ids.data_ptr() if len(ids_) else None, ids_len=len(ids_), off=d_off.data_ptr(), nseq=len(off_) - 1, flags=0, h=vp(hm))
    a.update(kw)
    p = [None if o is None else o.data_ptr() for o in outs]
    return bf.lib().IdsToMinHashBatchDevice(a["h"], a["ids"], a["ids_len"], a["off"], a["nseq"], k, H, r, seed, a["flags"], p[0], sig_cap, p[1], p[2], None)


def check_device(hm, ids, off, k, H, r, seed, want=None, sig_cap=None, take=(True, True, True)):
    """one call over canary-filled buffers: what the specification says is written equals the restatement, every byte around it is untouched,
    the status word is the restatement's; -> the buffers' bytes"""
    want = want or mc.restate(ids, off, k, H, r, seed)
    nseq, B = len(off) - 1, H // r if r else 0
    cap = nseq if sig_cap is None else sig_cap
    take = (take[0], take[1] and r > 0, take[2])
    bufs = [torch.full(((n + 64) * w,), CANARY, dtype=torch.uint8, device="cuda") for n, w in ((cap * H, 4), (cap * B, 8), (nseq, 4))]
    assert device_call(hm, ids, off, k, H, r, seed, [b if t else None for b, t in zip(bufs, take)], cap) == 0
    st = status(hm)
    got = [b.cpu().numpy() for b in bufs]
    for name, g, n, w, t in zip(("sig", "keys", "nshingles"), got, (min(nseq, cap) * H, min(nseq, cap) * B, nseq), (4, 8, 4), take):
        n = n if t else 0
        assert n == 0 or np.array_equal(g[:n * w], np.ascontiguousarray(want[name]).reshape(-1)[:n].view(np.uint8)), name
        assert (g[n * w:] == CANARY).all(), name
    assert st == (want["status"] | int(nseq > cap and take[0]))
    return got


@pytest.mark.parametrize("k,H,r,seed,base", mc.table())
def test_shapes(h, k, H, r, seed, base):
    check_device(h, *mc.ragged(mc.lengths(k), k * 1000 + H, base), k, H, r, seed)


def test_atomic_path_determinism_and_reserve(h):
    ids, off = mc.big()
    want = mc.restate(ids, off, 5, 65, 0, 5)
    fresh = bf.load_model(bfutil.model_path("bert_base_tok.i2w"))
    try:
        assert bf.lib().BfReserve(vp(fresh), len(off) - 1, 1 << 12, 0) == 0
        grows = bf.workspace_grows()
        a = check_device(fresh, ids, off, 5, 65, 0, 5, want)
        assert bf.workspace_grows() == grows, "the first call on the reserved handle allocated device memory"
    finally:
        bf.free_model(fresh)
    b = check_device(h, ids, off, 5, 65, 0, 5, want)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    for seed in (6, 7):                                         # two further seeds, each run twice: equal byte for byte, and not seed 5's
        sig = torch.empty((2, len(off) - 1, 65), dtype=torch.int32, device="cuda")
        assert [device_call(h, ids, off, 5, 65, 0, seed, [s, None, None], len(off) - 1) for s in sig] == [0, 0]
        assert torch.equal(sig[0], sig[1]) and sig[0].cpu().numpy().tobytes() != a[0][:sig[0].numel() * 4].tobytes()
    ms = bf.last_kernel_ms(h)
    assert ms[4] >= ms[1] > 0


@pytest.mark.parametrize("r", [1, 4, 128])
def test_band_keys(h, r):
    ids, off = mc.ragged([40, 40, 0, 7, 0], 21)
    ids[40:80] = ids[:40]                                       # two identical sequences; two empty ones, whose words are all equal
    want = mc.restate(ids, off, 5, 128, r, 77)
    check_device(h, ids, off, 5, 128, r, 77, want)
    assert np.array_equal(want["keys"][0], want["keys"][1]) and not np.array_equal(want["keys"][0], want["keys"][3])
    assert r == 128 or want["keys"][2][0] != want["keys"][2][1]                  # equal words, different bands: different keys


def test_cap_null_outputs_empty_batches_and_refusals(h):
    k, H, r = 5, 200, 4
    ids, off = mc.ragged(mc.lengths(k), 99)
    off[7] = off[8] + 1                                         # a decreasing range: status bit 3; the range before it now overlaps its successors
    want = mc.restate(ids, off, k, H, r, 1)
    for cap in (0, 1, 17, len(off) - 2):
        check_device(h, ids, off, k, H, r, 1, want, sig_cap=cap)
    check_device(h, ids, off, k, H, r, 1, want, sig_cap=0, take=(False, False, True))
    none = np.zeros(0, dtype=np.int32)
    check_device(h, none, np.zeros(1, dtype=np.int64), k, H, r, 1)               # nseq = 0
    check_device(h, none, np.zeros(131, dtype=np.int64), k, H, r, 1)             # ids_len = 0, nseq > 0
    check_device(h, ids, off, k, H, r, 1, want, take=(True, False, False))
    assert want["status"] == 8 == status(h)                     # the word every refusal below must leave alone
    outs = [torch.zeros(len(off) * 256, dtype=torch.int32, device="cuda"), None, None]
    for k_, H_, r_, kw in ((0, H, 0, {}), (9, H, 0, {}), (k, 0, 0, {}), (k, 257, 0, {}), (k, H, -1, {}), (k, H, 3, {}), (k, H, 0, dict(flags=1)), (k, H, 0, dict(nseq=-1)),
                           (k, H, 0, dict(nseq=1 << 31)), (k, H, 0, dict(ids_len=-1)), (k, H, 0, dict(off=None)), (k, H, 0, dict(ids=None)), (k, H, 0, dict(h=None))):
        assert device_call(h, ids, off, k_, H_, r_, 0, outs, len(off) - 1, **kw) == -1, (k_, H_, r_, kw)
    assert device_call(h, ids, off, k, H, 0, 0, outs, -1) == -1 and device_call(h, ids, off, k, H, 0, 0, [None] * 3, 3) == -1
    assert device_call(h, ids, off, k, H, 0, 0, [outs[0], outs[0], None], 3) == -1 and status(h) == 8


@pytest.mark.parametrize("nseq", [0, 3, None])
def test_host_form(h, nseq):
    ids, off = mc.ragged(mc.lengths(5), 4, 3)
    off = off[:len(off) if nseq is None else nseq + 1]
    want = mc.restate(ids, off, 5, 65, 5, 9)
    for g, name in zip(bf.ids_to_minhash_batch(h, ids, off, 65, 5, 5, 9), ("sig", "keys", "nshingles")):
        assert g.dtype == want[name].dtype and np.array_equal(g, want[name]), name
    sig, nsh = np.full((2, 65), CANARY, dtype=np.int32), np.zeros(len(off) - 1, dtype=np.int32)
    r = bf.lib().IdsToMinHashBatch(vp(h), ids.ctypes.data, off.ctypes.data, len(off) - 1, 5, 65, 0, 9, 0, sig.ctypes.data, 2, None, nsh.ctypes.data)
    assert (r == -3 and (sig == CANARY).all() if len(off) > 3 else r == len(off) - 1) and np.array_equal(nsh, want["nshingles"])


@pytest.mark.parametrize("H", [1, 20, 32, 64, 65, 256])
def test_pairs(h, H):
    sig = np.random.default_rng(H).integers(-(1 << 31), 1 << 31, size=(9, H)).astype(np.int32)
    sig[1], sig[2, :1], sig[3, :H - 1] = sig[0], sig[0, :1], sig[0, :H - 1]       # H, 1 and H - 1 equal slots; row 4 has none
    pairs = np.array([[0, 1], [0, 2], [0, 3], [0, 4], [5, 5], [3, 2], [0, 9], [-1, 0], [8, 7]], dtype=np.int64)
    want = np.array([(sig[a] == sig[b]).sum() if 0 <= a < 9 and 0 <= b < 9 else -1 for a, b in pairs], dtype=np.int32)
    assert H == 1 or want[:5].tolist() == [H, 1, H - 1, 0, H]
    d_sig, d_pairs = torch.from_numpy(sig).cuda(), torch.from_numpy(pairs).cuda()
    assert np.array_equal(bf.minhash_pairs_device(h, d_sig, d_pairs).cpu().numpy(), want) and status(h) == 8
    assert np.array_equal(bf.minhash_pairs_device(h, d_sig, d_pairs[:6]).cpu().numpy(), want[:6]) and status(h) == 0


@pytest.mark.parametrize("model", sorted(rc.ENCODE_MODELS))
def test_text_to_signatures(model):
    ref_ids, ref_off = rc.fixture_ids(rc.load_fixture(), model, 14)              # the stored reference ids at max_len 14
    want = mc.restate(ref_ids, ref_off, 3, 64, 8, 2)
    hm = bf.load_model(bfutil.model_path(model))
    try:
        d_text, d_off = (torch.from_numpy(x.copy()).cuda() for x in bf.pack_docs(rc.encode_docs()))
        got = bf.encode_minhash_batch_device(hm, d_text, d_off, 14, 64, 3, 8, 2, unk=rc.ENCODE_MODELS[model]["unk"])
        assert status(hm) == 0 and all(np.array_equal(g.cpu().numpy(), want[name]) for g, name in zip(got, ("sig", "keys", "nshingles")))
    finally:
        bf.free_model(hm)
