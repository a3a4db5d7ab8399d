"""TEST helpers for IdsToRowsBatch: a numpy restatement of the specification in include/blingfiretokdll_amd.h (written from that text, one
row at a time, not from blingfire_amd/csrc/bf_rows.h), the parameter table the CPU and GPU tiers share, and the stored reference ids
of the end-to-end cases (tests/golden/rows/encode_ids.json, written by tests/golden/make_rows_fixture.py)."""
import itertools
import json
import os

import numpy as np

import bfutil

FIXTURE = os.path.join(bfutil.ROOT, "tests", "golden", "rows", "encode_ids.json")
INT32_MAX = 2 ** 31 - 1


def geometry(L, cls_id, sep_id, stride):
    """(body, step) or None when the call must answer BF_E_ARG"""
    body = L - (1 if cls_id >= 0 else 0) - (1 if sep_id >= 0 else 0)
    if L < 1 or L > 1 << 20 or body < 1 or stride < 0 or stride >= body:
        return None
    return body, body - stride


def restate(ids, id_off, L, cls_id=-1, sep_id=-1, pad_id=0, stride=0, max_rows=1, pad_left=False, ids_len=None):
    """-> (rows int32[R, L], mask uint8[R, L], row_seq int32[R], row_first int32[R], row_offsets int64[nseq+1], status)"""
    body, step = geometry(L, cls_id, sep_id, stride)
    ids = np.asarray(ids, dtype=np.int32)
    id_off = [int(x) for x in id_off]
    if ids_len is None:
        ids_len = len(ids)
    rows, mask, seqs, firsts, offs, status = [], [], [], [], [0], 0
    for q in range(len(id_off) - 1):
        b, e = id_off[q], id_off[q + 1]
        if b < 0 or e < b or e > ids_len:                 # not inside [0, ids_len], or decreasing: an empty sequence, bit 3
            status |= 8
            tok = ids[:0]
        else:
            tok = ids[b:e]
        n = len(tok)
        nrows = 1 if n <= body else 1 + -(-(n - body) // step)
        if max_rows > 0:
            nrows = min(nrows, max_rows)
        for w in range(nrows):
            win = tok[w * step:min(n, w * step + body)]
            real = ([cls_id] if cls_id >= 0 else []) + [int(x) for x in win] + ([sep_id] if sep_id >= 0 else [])
            pad = [pad_id] * (L - len(real))
            rows.append(pad + real if pad_left else real + pad)
            mask.append([0] * len(pad) + [1] * len(real) if pad_left else [1] * len(real) + [0] * len(pad))
            seqs.append(q)
            firsts.append(w * step)
        offs.append(offs[-1] + nrows)
    return (np.array(rows, dtype=np.int32).reshape(-1, L), np.array(mask, dtype=np.uint8).reshape(-1, L), np.array(seqs, dtype=np.int32),
            np.array(firsts, dtype=np.int32), np.array(offs, dtype=np.int64), status)


def restate_truncated(ids, id_off, L, cls_id, sep_id, pad_id):
    """restate(..., stride=0, max_rows=1, pad_left=False) with both specials present, as array operations (for batches too large for the
    row-at-a-time form; tests/test_rows_host.py holds it to that form): -> (rows, mask, row_seq, row_first, row_offsets)"""
    ids = np.asarray(ids, dtype=np.int32)
    id_off = np.asarray(id_off, dtype=np.int64)
    nseq = len(id_off) - 1
    k = np.minimum(np.diff(id_off), L - 2)[:, None]      # ids kept per sequence
    j = np.arange(L, dtype=np.int64)[None, :]
    is_id = (j >= 1) & (j <= k)
    src = np.where(is_id, id_off[:-1, None] + j - 1, 0)
    rows = np.where(is_id, ids[src] if len(ids) else 0, pad_id).astype(np.int32)
    rows[:, 0] = cls_id
    rows[np.arange(nseq), k[:, 0] + 1] = sep_id
    return rows, (j <= k + 1).astype(np.uint8), np.arange(nseq, dtype=np.int32), np.zeros(nseq, dtype=np.int32), np.arange(nseq + 1, dtype=np.int64)


CLS, SEP, PAD = 101, 102, 0
TABLE_L = [1, 2, 3, 4, 5, 8, 63, 64, 130]


def table_lengths(body, step):
    return [0, 1, body - 1, body, body + 1, body + step, body + step + 1, 3 * body + 1]


def table():
    """every parameter combination of the table: (L, cls_id, sep_id, stride, max_rows, pad_left).  L = 1 only without specials, every
    other L with each special present and absent; a stride the body has no room for (and a repeated one) is left out."""
    out = []
    for L in TABLE_L:
        for cls_id, sep_id in ([(-1, -1)] if L == 1 else itertools.product((CLS, -1), (SEP, -1))):
            g = geometry(L, cls_id, sep_id, 0)
            if g is None:
                continue
            body = g[0]
            for stride in sorted({0, 1, body - 1}):
                if geometry(L, cls_id, sep_id, stride) is None:
                    continue
                for max_rows in (0, 1, 2, 3):
                    for pad_left in (False, True):
                        out.append((L, cls_id, sep_id, stride, max_rows, pad_left))
    return out


def synthetic(body, step, seed=0):
    """ragged ids with the table's sequence lengths (ids 1000.. so that no id equals a special or the padding)"""
    lens = table_lengths(body, step)
    off = np.zeros(len(lens) + 1, dtype=np.int64)
    np.cumsum(lens, out=off[1:])
    ids = (1000 + seed + np.arange(int(off[-1]))).astype(np.int32)
    return ids, off


# ---- the end-to-end cases: (L, stride, max_rows_per_doc, pad_left) and the TextToIds max_len encode_batch_device derives from each
ENCODE_CASES = [(16, 0, 1, False), (16, 4, 0, False), (8, 0, 1, True)]
ENCODE_MODELS = {"bert_base_tok.bin": dict(cls_id=101, sep_id=102, pad_id=0, unk=100), "gpt2.bin": dict(cls_id=50256, sep_id=50256, pad_id=50256, unk=0)}


def encode_max_len(L, stride, max_rows):
    body = L - 2
    return body + (max_rows - 1) * (body - stride) if max_rows > 0 else INT32_MAX


def encode_docs():
    return list(bfutil.ADVERSARIAL) + bfutil.fuzz_docs(48)


def load_fixture():
    with open(FIXTURE) as f:
        return json.load(f)


def fixture_ids(fx, model, max_len):
    """(ids int32, id_offsets int64) of the stored reference answers of `model` at `max_len`"""
    per_doc = fx["models"][model][str(max_len)]
    off = np.zeros(len(per_doc) + 1, dtype=np.int64)
    np.cumsum([len(d) for d in per_doc], out=off[1:])
    ids = np.array([i for d in per_doc for i in d], dtype=np.int32)
    return ids, off
