"""CPU: what the bucketed wrappers send to the C library, call by call, against the recording stand-in of test_wrapper_calls.py (no built
library, model or device), and how bucketed_views cuts the flat planes up."""
import numpy as np

from test_wrapper_calls import IDS, N, OFF, P, dev_docs, dev_ragged, env, put64, raises, shapes  # noqa: F401  (env is the fixture)

ARGS = (8, 101, 102, 0, 8, 64, 0, 0)                       # max_len, cls, sep, pad, multiple, max_cells, max_rows, flags


def writes_counts(at, B, C, ret=0):
    def f(*args):
        put64(args[at], 0, B)
        put64(args[at], 1, C)
        return ret
    return f


def outs(nseq, B, C):
    return [((C,), "int32"), ((C,), "uint8"), ((nseq,), "int32"), ((nseq,), "int32"), ((B + 1,), "int32"), ((B + 1,), "int32"), ((B + 1,), "int64"), ((2,), "int64")]


def test_host_form_asks_for_its_size_first(env):
    bf, L = env.bf, env.L
    L.script["IdsToBucketedRowsBatch"] = [writes_counts(21, 2, 16, 16), 16, -3]
    assert shapes(bf.ids_to_bucketed_rows_batch(7, IDS, OFF, 8, 64, 101, 102)) == outs(2, 2, 16)
    raises(RuntimeError, "IdsToBucketedRowsBatch failed: -3 (boom)", bf.ids_to_bucketed_rows_batch, 7, IDS, OFF, 8, 64)
    pre = (P, P, P, 2) + ARGS
    assert L.log[:2] == [("IdsToBucketedRowsBatch", pre + (N, N, 0, P, P, N, N, N, 0, P)), ("IdsToBucketedRowsBatch", pre + (P, P, 16, P, P, P, P, P, 2, P))]
    assert L.log[2] == ("IdsToBucketedRowsBatch", (P, P, P, 2, 8, -1, -1, 0, 8, 64, 0, 0, N, N, 0, P, P, N, N, N, 0, P))


def test_device_form_reads_back_only_without_caps(env):
    bf, L, torch = env.bf, env.L, env.torch
    d_ids, d_off = dev_ragged(torch)
    L.script["IdsToBucketedRowsBatchDevice"] = [writes_counts(22, 2, 16), 0, 0, writes_counts(22, 3, 24), 0, -2]
    pre = (P, P, 3, P, 2) + ARGS
    assert shapes(bf.ids_to_bucketed_rows_batch_device(7, d_ids, d_off, 8, 64, 101, 102, stream=9)) == outs(2, 2, 16)
    assert shapes(bf.ids_to_bucketed_rows_batch_device(7, d_ids, d_off, 8, 64, 101, 102, cells_cap=40, batches_cap=5)) == outs(2, 5, 40)
    assert shapes(bf.ids_to_bucketed_rows_batch_device(7, d_ids, d_off, 8, 64, 101, 102, batches_cap=9)) == outs(2, 9, 24)
    raises(RuntimeError, "IdsToBucketedRowsBatchDevice failed (-2): boom", bf.ids_to_bucketed_rows_batch_device, 7, d_ids, d_off, 8, 64, cells_cap=1, batches_cap=1)
    query, full = pre + (N,) * 2 + (0,) + (N,) * 5 + (0, P, P), lambda C, B: pre + (P, P, C, P, P, P, P, P, B, P, P)
    assert [e for e in L.log if e[0] != "BfLastError"] == [
        ("IdsToBucketedRowsBatchDevice", query), ("<sync>", ()), ("IdsToBucketedRowsBatchDevice", full(16, 2)), ("IdsToBucketedRowsBatchDevice", full(40, 5)),
        ("IdsToBucketedRowsBatchDevice", query), ("IdsToBucketedRowsBatchDevice", full(24, 9)),
        ("IdsToBucketedRowsBatchDevice", (P, P, 3, P, 2, 8, -1, -1, 0, 8, 64, 0, 0, P, P, 1, P, P, P, P, P, 1, P, P))]
    assert env.streams                                          # without `stream`: torch's current stream


def test_encode_runs_the_tokenizer_up_to_body(env):
    bf, L, torch = env.bf, env.L, env.torch
    d_text, d_off = dev_docs(torch)
    got = bf.encode_bucketed_batch_device(7, d_text, d_off, 8, 101, 102, 0, 64, multiple=4, max_rows=3, unk=5, cells_cap=32, batches_cap=2)
    assert shapes(got) == outs(2, 2, 32)
    assert L.log == [("TextToIdsBatchDevice", (P, P, P, 2, 3, P, 10, P, 6, 5, P)),
                     ("IdsToBucketedRowsBatchDevice", (P, P, 10, P, 2, 8, 101, 102, 0, 4, 64, 3, 0, P, P, 32, P, P, P, P, P, 2, P, P))]
    raises(ValueError, "encode_bucketed_batch_device: max_len leaves no room for ids", bf.encode_bucketed_batch_device, 7, d_text, d_off, 2, 101, 102, 0, 64)


def test_bucketed_views(env):
    torch = env.torch
    rows, mask = np.arange(12, dtype=np.int32), np.ones(12, dtype=np.uint8)
    per_batch = (np.array([0, 1, 3, 0], dtype=np.int32), np.array([4, 3, 0, 0], dtype=np.int32), np.array([0, 4, 10, 0], dtype=np.int64), np.array([2, 10], dtype=np.int64))
    for conv in (lambda a: a, torch.from_numpy):
        views = list(env.bf.bucketed_views(conv(rows), conv(mask), *map(conv, per_batch)))
        assert [(tuple(r.shape), tuple(m.shape), s) for r, m, s in views] == [((1, 4), (1, 4), slice(0, 1)), ((2, 3), (2, 3), slice(1, 3))]
        assert np.asarray(views[1][0]).tolist() == [[4, 5, 6], [7, 8, 9]]
    cut = list(env.bf.bucketed_views(rows[:8], mask[:8], *per_batch))       # a cells_cap that ends inside batch 1
    assert len(cut) == 1
