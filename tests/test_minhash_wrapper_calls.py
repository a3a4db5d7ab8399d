"""CPU: what the MinHash wrappers send to the C library, call by call, against the recording stand-in of test_wrapper_calls.py."""
from test_wrapper_calls import IDS, N, OFF, P, dev_docs, dev_ragged, env, raises, shapes  # noqa: F401  (env is the fixture)

SEED = (1 << 64) - 1


def outs(nseq, H, B):
    return [((nseq, H), "int32")] + ([((nseq, B), "int64")] if B else []) + [((nseq,), "int32")]


def some(out):
    return shapes([x for x in out if x is not None])


def test_host_form(env):
    bf, L = env.bf, env.L
    L.script["IdsToMinHashBatch"] = [2, 2, -3]
    assert some(bf.ids_to_minhash_batch(7, IDS, OFF)) == outs(2, 128, 0)
    assert some(bf.ids_to_minhash_batch(7, IDS, OFF, num_perm=64, shingle=3, band_rows=4, seed=-1)) == outs(2, 64, 16)
    raises(RuntimeError, "IdsToMinHashBatch failed: -3 (boom)", bf.ids_to_minhash_batch, 7, IDS, OFF)
    assert L.log[:2] == [("IdsToMinHashBatch", (P, P, P, 2, 5, 128, 0, 0, 0, P, 2, N, P)), ("IdsToMinHashBatch", (P, P, P, 2, 3, 64, 4, SEED, 0, P, 2, P, P))]


def test_device_forms(env):
    bf, L, torch = env.bf, env.L, env.torch
    d_ids, d_off = dev_ragged(torch)
    L.script["IdsToMinHashBatchDevice"] = [0, -2, 0]
    sig, keys, nsh = bf.ids_to_minhash_batch_device(7, d_ids, d_off, stream=9)
    assert keys is None and shapes((sig, nsh)) == outs(2, 128, 0)
    raises(RuntimeError, "IdsToMinHashBatchDevice failed (-2): boom", bf.ids_to_minhash_batch_device, 7, d_ids, d_off, 256, 8, 256, SEED)
    assert shapes([bf.minhash_pairs_device(7, sig, torch.tensor([[0, 1], [1, 1], [0, 5]], dtype=torch.int64))]) == [((3,), "int32")]
    assert some(bf.encode_minhash_batch_device(7, *dev_docs(torch), 6, num_perm=64, shingle=2, band_rows=8, seed=3, unk=5)) == outs(2, 64, 8)
    assert [e for e in L.log if e[0] != "BfLastError"] == [
        ("IdsToMinHashBatchDevice", (P, P, 3, P, 2, 5, 128, 0, 0, 0, P, 2, N, P, P)), ("IdsToMinHashBatchDevice", (P, P, 3, P, 2, 8, 256, 256, SEED, 0, P, 2, P, P, P)),
        ("MinHashPairsBatchDevice", (P, P, 128, 2, P, 3, P, P)), ("TextToIdsBatchDevice", (P, P, P, 2, 3, P, 10, P, 6, 5, P)),
        ("IdsToMinHashBatchDevice", (P, P, 10, P, 2, 2, 64, 8, 3, 0, P, 2, P, P, P))]
    assert env.streams                                          # without `stream`: torch's current stream
