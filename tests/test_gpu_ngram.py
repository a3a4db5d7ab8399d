"""GPU: IdsToNgramSetBatchDevice and IdsNgramOverlapBatchDevice (bf_kernels_ngram.hip) and the Python calls above them against the sequential
restatement of the specification (ngram_cases), byte for byte over canary-filled buffers."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import bfutil
import blingfire_amd as bf
import minhash_cases as mc
import ngram_cases as nc

pytestmark = pytest.mark.gpu
CANARY, SEED = 0x5A, 0x0123456789ABCDEF
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
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def set_call(hm, ids, off, n, table, flags=1, seed=SEED, **kw):
    """-> (return value, counts); kw replaces arguments of the call by name"""
    d_ids, d_off, counts = dev(ids), dev(off), torch.full((3,), -7, dtype=torch.int64, device="cuda")
    a = dict(h=vp(hm), p_ids=d_ids.data_ptr(), ids_len=len(ids), p_off=d_off.data_ptr(), nseq=len(off) - 1, ngram=n, flag=flags, tab=table.data_ptr(), slots=table.numel(),
             counts=counts.data_ptr())
    a.update(kw)
    r = bf.lib().IdsToNgramSetBatchDevice(a["h"], a["p_ids"], a["ids_len"], a["p_off"], a["nseq"], a["ngram"], seed, a["flag"], a["tab"], a["slots"], a["counts"], None)
    return r, counts.cpu().numpy()


def check_overlap(hm, ids, off, n, table, members, take=(1, 1, 1, 1), seed=SEED):
    """one overlap call over canary-filled buffers: the outputs taken equal the restatement, every other byte is untouched"""
    want = nc.overlap(ids, off, n, seed, members)
    nseq, d_ids, d_off = len(off) - 1, dev(ids), dev(off)
    bufs = [torch.full((w * (m + 64),), CANARY, dtype=torch.uint8, device="cuda") for m, w in ((nseq, 4), (nseq, 4), (nseq, 4), (len(ids), 1))]
    p = [b.data_ptr() if t else None for b, t in zip(bufs, take)]
    assert bf.lib().IdsNgramOverlapBatchDevice(vp(hm), d_ids.data_ptr(), len(ids), d_off.data_ptr(), nseq, n, seed, 0, table.data_ptr(), table.numel(), *p, None) == 0
    assert status(hm) == want["status"]
    for name, b, t in zip(("ngrams", "hits", "covered", "mask"), bufs, take):
        w = np.where(want["mask"] == 7, CANARY, want["mask"]) if name == "mask" else want[name].view(np.uint8)
        assert np.array_equal(b.cpu().numpy(), np.concatenate([w, np.full(len(b) - len(w), CANARY, np.uint8)]) if t else np.full(len(b), CANARY, np.uint8)), name
    return want


@pytest.mark.parametrize("n", nc.NS)
def test_case_table(h, n):
    ids, off, s_ids, s_off = nc.case(n)
    members, want_counts = nc.build(s_ids, s_off, n, SEED)
    table = torch.full((len(members) + 1,), CANARY, dtype=torch.int64, device="cuda")         # one slot to spare: the probes wrap around the end
    r, counts = set_call(h, s_ids, s_off, n, table)
    assert r == 0 and status(h) == 0 and counts.tolist() == want_counts.tolist()
    want = check_overlap(h, ids, off, n, table, members)
    assert want["status"] == 8 and want["hits"].sum() > 0 and (want["hits"] < want["ngrams"]).any()
    # the batch against its own set: every n-gram hits, every id of a sequence that has one is covered
    own, _ = nc.build(ids, off, n, SEED)
    table, counts = bf.ngram_set_device(h, dev(ids), dev(off), n, SEED)
    ng, hits, cov = (x.cpu().numpy() for x in bf.ngram_overlap_device(h, dev(ids), dev(off), table, n, SEED))
    lens = np.where(ng > 0, ng + n - 1, 0)
    assert counts.cpu().tolist() == [int(ng.sum()), len(own), 0] and np.array_equal(hits, ng) and np.array_equal(cov, lens)


def test_two_calls_two_ns_one_table_and_a_table_too_small(h):
    ids, off, s_ids, s_off = nc.case(13)
    half = len(s_off) // 2
    a_off, b_off = s_off[:half + 1], s_off[half:]
    members, _ = nc.build(s_ids, s_off, 13, SEED)
    first, _ = nc.build(s_ids, a_off, 13, SEED)
    table = torch.full((2 * len(s_ids) + 64,), CANARY, dtype=torch.int64, device="cuda")
    assert set_call(h, s_ids, a_off, 13, table, 1)[0] == 0
    r, counts = set_call(h, s_ids, b_off, 13, table, 0)                            # added to what is there
    assert r == 0 and counts.tolist() == nc.build(s_ids, b_off, 13, SEED, first)[1].tolist()
    check_overlap(h, ids, off, 13, table, members)
    eight, c8 = nc.build(s_ids, s_off, 8, SEED)                                  # n is part of the fingerprint: the same table answers n = 8 too
    assert set_call(h, s_ids, s_off, 8, table, 0)[1].tolist() == c8.tolist()
    check_overlap(h, ids, off, 13, table, members | eight)
    check_overlap(h, ids, off, 8, table, members | eight)
    small = torch.zeros(len(members) - 3, dtype=torch.int64, device="cuda")
    r, counts = set_call(h, s_ids, s_off, 13, small)
    assert r == 0 and counts[2] > 0 and status(h) & 1


def test_null_outputs_and_refusals(h):
    ids, off, s_ids, s_off = nc.case(2)
    ids, off = ids[:int(off[40])], off[:41]
    members, _ = nc.build(s_ids, s_off, 2, SEED)
    table, _ = bf.ngram_set_device(h, dev(s_ids), dev(s_off), 2, SEED)
    for take in itertools.product((0, 1), repeat=4):
        if any(take):
            check_overlap(h, ids, off, 2, table, members, take)
    bf.minhash_pairs_device(h, torch.zeros((1, 4), dtype=torch.int32, device="cuda"), torch.tensor([[0, 1]], dtype=torch.int64, device="cuda"))
    assert status(h) == 8                                                      # a status word for the refusals to leave alone
    before = table.clone()
    for kw in (dict(ngram=0), dict(ngram=65), dict(slots=1), dict(tab=None), dict(p_off=None), dict(h=None), dict(nseq=-1), dict(nseq=1 << 31), dict(ids_len=-1),
               dict(p_ids=None), dict(flag=2), dict(counts=None)):
        assert set_call(h, s_ids, s_off, 2, table, **kw)[0] == -1, kw
    d_ids, d_off, out = dev(ids), dev(off), torch.zeros(40, dtype=torch.int32, device="cuda")
    for args in ((0, SEED, 0, table.data_ptr(), 70), (65, SEED, 0, table.data_ptr(), 70), (2, SEED, 1, table.data_ptr(), 70), (2, SEED, 0, None, 70), (2, SEED, 0, table.data_ptr(), 1)):
        assert bf.lib().IdsNgramOverlapBatchDevice(vp(h), d_ids.data_ptr(), len(ids), d_off.data_ptr(), 40, *args, out.data_ptr(), None, None, None, None) == -1
    assert bf.lib().IdsNgramOverlapBatchDevice(vp(h), d_ids.data_ptr(), len(ids), d_off.data_ptr(), 40, 2, SEED, 0, table.data_ptr(), 70, None, None, None, None, None) == -1
    assert status(h) == 8 and torch.equal(table, before) and (out == 0).all()


def test_between_two_minhash_calls_on_a_reserved_handle():
    ids, off, s_ids, s_off = nc.case(13)
    ids, off = ids[:int(off[-2])], off[:-1]                                     # (without the bad range)
    want = mc.restate(ids[:int(off[20])], off[:21], 3, 64, 4, 2)
    fresh = bf.load_model(bfutil.model_path("bert_base_tok.i2w"))
    try:
        assert bf.lib().BfReserve(vp(fresh), len(off) - 1, 1 << 12, 0) == 0
        grows = bf.workspace_grows()
        table, _ = bf.ngram_set_device(fresh, dev(s_ids), dev(s_off), 13, SEED)
        a = bf.ids_to_minhash_batch_device(fresh, dev(ids), dev(off), 64, 3, 4, 2)
        check_overlap(fresh, ids, off, 13, table, nc.build(s_ids, s_off, 13, SEED)[0])
        b = bf.ids_to_minhash_batch_device(fresh, dev(ids), dev(off), 64, 3, 4, 2)
        assert bf.workspace_grows() == grows, "a call on the reserved handle allocated device memory"
        assert all(torch.equal(x, y) for x, y in zip(a, b)) and np.array_equal(a[0][:20].cpu().numpy(), want["sig"][:20])
    finally:
        bf.free_model(fresh)
