"""GPU: MinHashClustersBatchDevice (bf_kernels_mhclust.hip) and the Python calls above it against the sequential restatement of the specification
(mhclust_cases.restate), by exact equality over canary-filled buffers."""
import ctypes

import numpy as np
import pytest
import torch

import bfutil
import blingfire_amd as bf
import mhclust_cases as cc
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


def dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def device_call(hm, d_keys, d_sig, d_nsh, outs, **kw):
    """kw: H, B, nseq, min_equal, and whatever else of the call's arguments is to be replaced"""
    a = dict(h=vp(hm), sig=bf._dev_addr(d_sig), keys=bf._dev_addr(d_keys), flags=0)
    a.update(kw)
    p = [bf._dev_addr(o) for o in outs]
    return bf.lib().MinHashClustersBatchDevice(a["h"], a["sig"], a["H"], a["keys"], a["B"], a["nseq"], bf._dev_addr(d_nsh), a["min_equal"], a["flags"], *p, None)


def check_device(hm, keys, sig, min_equal, nsh, want, take=(True, True)):
    """one call over canary-filled buffers: label, keep, size and counts equal the restatement, every byte behind them is untouched, the status
    word is 0; -> the buffers' bytes"""
    nseq, B = keys.shape
    bufs = [torch.full(((n + 64) * w,), CANARY, dtype=torch.uint8, device="cuda") for n, w in ((nseq, 4), (nseq, 1), (nseq, 4), (2, 8))]
    outs = [bufs[0], bufs[1] if take[0] else None, bufs[2] if take[1] else None, bufs[3]]
    assert device_call(hm, dev(keys), dev(sig), dev(nsh), outs, H=1 if sig is None else sig.shape[1], B=B, nseq=nseq, min_equal=min_equal) == 0
    assert status(hm) == 0
    got = [b.cpu().numpy() for b in bufs]
    for name, g, o in zip(("label", "keep", "size", "counts"), got, outs):
        n = want[name].nbytes if o is not None else 0
        assert np.array_equal(g[:n], want[name].view(np.uint8)[:n]), name
        assert (g[n:] == CANARY).all(), name
    return got


@pytest.mark.parametrize("nseq,B,H,min_equal", cc.table())
def test_random_table(h, nseq, B, H, min_equal):
    keys, sig, nsh, want = cc.random_case(nseq, B, H, min_equal)
    check_device(h, keys, sig, min_equal, nsh, want)


@pytest.mark.parametrize("name", cc.NAMED)
def test_named_shapes(h, name):
    keys, says = cc.named(name)
    want = cc.restate(keys)
    assert want["counts"].tolist() == [says["clusters"], says["candidates"]]
    check_device(h, keys, None, 0, None, want)


def test_reserve_determinism_null_outputs_empty_batch_and_refusals(h):
    nseq, B, H, me = 1000, 5, 20, 10
    keys, sig, nsh, want = cc.random_case(nseq, B, H, me)
    fresh = bf.load_model(bfutil.model_path("bert_base_tok.i2w"))
    try:
        assert bf.lib().BfReserve(vp(fresh), nseq, 1 << 12, 0) == 0
        grows = bf.workspace_grows()
        a = check_device(fresh, keys, sig, me, nsh, want)
        assert bf.workspace_grows() == grows, "the first call on the reserved handle allocated device memory"
    finally:
        bf.free_model(fresh)
    b = check_device(h, keys, sig, me, nsh, want)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    ms = bf.last_kernel_ms(h)
    assert ms[4] >= ms[1] > 0
    for take in ((False, False), (True, False), (False, True)):
        check_device(h, keys, sig, me, nsh, want, take)
    check_device(h, keys, None, 0, None, cc.restate(keys))                       # no signatures, every sequence live
    check_device(h, keys[:0], sig[:0], me, nsh[:0], cc.restate(keys[:0], sig[:0], me, nsh[:0]))      # nseq = 0: counts = {0, 0}
    # a status word for the refusals to leave alone: a pair outside [0, nseq) sets bit 3
    d_keys, d_sig, d_nsh = dev(keys), dev(sig), dev(nsh)
    bf.minhash_pairs_device(h, d_sig, torch.tensor([[0, nseq]], dtype=torch.int64, device="cuda"))
    assert status(h) == 8
    outs = [torch.zeros(nseq, dtype=torch.int32, device="cuda"), None, None, torch.zeros(2, dtype=torch.int64, device="cuda")]
    good = dict(H=H, B=B, nseq=nseq, min_equal=me)
    for kw in (dict(H=0), dict(H=257), dict(B=0), dict(B=257), dict(min_equal=-1), dict(min_equal=H + 1), dict(flags=1), dict(nseq=-1), dict(nseq=(1 << 31) - 1),
               dict(h=None), dict(keys=None), dict(sig=None)):
        assert device_call(h, d_keys, d_sig, d_nsh, outs, **dict(good, **kw)) == -1, kw
    assert device_call(h, d_keys, d_sig, d_nsh, [None] + outs[1:], **good) == -1
    assert device_call(h, d_keys, d_sig, d_nsh, outs[:3] + [None], **good) == -1
    assert device_call(h, d_keys, d_sig, d_nsh, outs[:3] + [None], **dict(good, nseq=0)) == -1 and status(h) == 8
    assert (outs[0] == 0).all() and (outs[3] == 0).all()


@pytest.mark.parametrize("model", sorted(rc.ENCODE_MODELS))
def test_text_to_clusters(model):
    docs = rc.encode_docs()
    n = len(docs)
    ref_ids, ref_off = rc.fixture_ids(rc.load_fixture(), model, 14)              # the stored reference ids at max_len 14
    # the corpus: every document, the first five again, and five more with one word put in front.  The ids of the first two parts are the stored
    # reference's; those of the changed documents (the reference stores none) are the tokenizer call's own, which test_gpu_rows holds to the reference
    pick = list(range(n)) + list(range(5))
    corpus = [docs[i] for i in pick] + [(b"zebra " if isinstance(docs[i], bytes) else "zebra ") + docs[i] for i in range(5, 10)]
    seqs = [ref_ids[ref_off[i]:ref_off[i + 1]] for i in pick]
    hm = bf.load_model(bfutil.model_path(model))
    try:
        d_text, d_off = (torch.from_numpy(x.copy()).cuda() for x in bf.pack_docs(corpus))
        t_ids, t_off = (x.cpu().numpy() for x in bf.text_to_ids_batch_device(hm, d_text, d_off, 14, rc.ENCODE_MODELS[model]["unk"]))
        seqs += [t_ids[t_off[i]:t_off[i + 1]] for i in range(len(pick), len(corpus))]
        ids, off = np.concatenate(seqs).astype(np.int32), np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.int64)
        mh = mc.restate(ids, off, 3, 64, 4, 2)
        for jac in (0.0, 0.5):
            me = int(np.ceil(jac * 64))
            want = cc.restate(mh["keys"], mh["sig"], me, mh["nshingles"])
            got = bf.encode_dedup_batch_device(hm, d_text, d_off, 14, 64, 3, 4, jac, 2, unk=rc.ENCODE_MODELS[model]["unk"])
            assert status(hm) == 0
            for g, w in zip(got, (want["label"], want["keep"].astype(bool), want["size"], want["counts"], mh["sig"], mh["nshingles"])):
                assert np.array_equal(g.cpu().numpy(), w)
            assert all(want["label"][n + i] == want["label"][i] for i in range(5) if mh["nshingles"][i] > 0)      # a repeated document joins its first copy
    finally:
        bf.free_model(hm)
