"""The contract the host-buffer batch calls share (bf_capi.cpp: stage_ragged, two_pass_host), on the parts of it no other test reaches, for
TextToWordsBatch, TextToSentencesBatch, IdsToTextBatch, NormalizeSpacesBatch, TextToHashesBatch, WordHyphenationBatch and DictGetInfoBatch
(IdsToRowsBatch: the first and the third):

  1  an offset array whose first entry is not zero: the batch starts at element 7 of a larger array whose elements in front of and behind it
     are valid input (words, ids, key symbols) that would show in the answer if they were read; the returned offsets start at 0;
  2  NULL *_offsets_out: the same return value and output;
  3  an empty batch: n = 0, the offset array [5], NULL payload and output: the call returns 0;
  4  a NULL output with a non-empty result and a sufficient capacity: BF_E_ARG, the offsets complete.

Every batch has five items; one is empty and one is longer than 64 elements (it crosses a kernel window).  The expectations are per item and
come from where tests/test_gpu_secondary_at_scale.py takes them: secondary_cases.Checker / DictChecker (the compiled reference where
oracle/_ref is built, else the oracle restatement), w2h_cases (the reference's answers, live or stored) and rows_cases.restate.  Every
comparison is exact."""
import ctypes

import numpy as np
import pytest

import bfutil
import rows_cases as rc
import secondary_cases as sc
import w2h_cases as wc

pytestmark = pytest.mark.gpu

E_ARG = -1
FIRST = 7                                                      # the batch's first offset
CANARY = {np.dtype(np.uint8): 0xA5, np.dtype(np.int32): 0x5A5A5A5A}
I64, VP, CI = ctypes.c_int64, ctypes.c_void_p, ctypes.c_int
DOCS = [b"Hello world. This is a test! Is it?", b"", b"One sentence here. And a second one, of a few words more. " * 3, "x　▁ y".encode(), b"ab  cd "]
AROUND_TEXT = (b"Zq x. Y", b" tail words. More")              # 7 bytes in front of the batch, 17 behind it
HOST_FORMS = ["TextToWordsBatch", "TextToSentencesBatch", "IdsToTextBatch", "NormalizeSpacesBatch", "TextToHashesBatch", "WordHyphenationBatch", "DictGetInfoBatch"]


def ptr(a):
    return None if a is None else a.ctypes.data


class Form:
    """One host entry point on one batch: fn(*head, payload, offsets, n, *per_item, output, capacity, offsets_out, *tail).
    per_item: DictGetInfoBatch's ret and info-id arrays with their expectations."""

    def __init__(self, fn, head, tail, items, want, around, in_dtype=np.uint8, out_dtype=np.uint8, per_item=()):
        self.fn, self.head, self.tail, self.n, self.per_item = fn, head, tail, len(items), per_item
        flat, off = sc.pack(items, in_dtype)
        front, back = (np.frombuffer(x, dtype=np.uint8) if isinstance(x, bytes) else np.asarray(x, dtype=in_dtype) for x in around)
        assert len(front) == FIRST and len(back) > 0 and any(len(x) == 0 for x in items) and any(len(x) > 64 for x in items) and self.n == 5
        self.inside = np.ascontiguousarray(np.concatenate([front, flat, back]).astype(in_dtype))
        self.off = off + FIRST
        self.want, self.want_off = sc.pack(want, out_dtype)
        self.T = int(self.want_off[-1])
        assert self.T > 0

    def call(self, payload, off, n, cap, with_out=True, with_off=True):
        out = np.full(max(cap, 0) + 64, CANARY[self.want.dtype], dtype=self.want.dtype)
        o_off = np.full(n + 1, -1, dtype=np.int64)
        extra = [np.full(max(n, 1), -77, dtype=np.int32) for _ in self.per_item]
        r = self.fn(*self.head, ptr(payload), ptr(off), n, *[ptr(e) if n else None for e in extra], ptr(out) if with_out else None, cap,
                    ptr(o_off) if with_off else None, *self.tail)
        return r, out, o_off, extra

    def check_output(self, r, out, extra):
        assert r == self.T
        assert np.array_equal(out[:self.T], self.want)
        assert (out[self.T:] == CANARY[self.want.dtype]).all()
        for got, want in zip(extra, self.per_item):
            assert np.array_equal(got, want)


@pytest.fixture(scope="module")
def forms():
    import blingfire_amd as bf
    L = bf.lib()
    L.NormalizeSpacesBatch.restype = L.TextToHashesBatch.restype = I64
    L.NormalizeSpacesBatch.argtypes = [VP, VP, I64, VP, I64, VP, CI]
    L.TextToHashesBatch.argtypes = [VP, VP, I64, VP, I64, VP, CI, CI]
    ck = sc.Checker()
    out, handles = {}, []
    out["TextToWordsBatch"] = Form(L.TextToWordsBatch, [None], [], DOCS, [ck.words(b) for b in DOCS], AROUND_TEXT)
    out["TextToSentencesBatch"] = Form(L.TextToSentencesBatch, [None], [], DOCS, [ck.sentences(b) for b in DOCS], AROUND_TEXT)
    out["NormalizeSpacesBatch"] = Form(L.NormalizeSpacesBatch, [], [0x2581], DOCS, [ck.normalize(b, 0x2581) for b in DOCS], AROUND_TEXT)
    out["TextToHashesBatch"] = Form(L.TextToHashesBatch, [], [2, 2000000], DOCS, [ck.hashes(b, 2, 2000000) for b in DOCS], AROUND_TEXT, out_dtype=np.int32)
    # ids to text: an unknown id (the sequence has no text), the leading-space rule, 100 ids
    ntok = sc.i2w_count("gpt2.i2w")
    seqs = [[5, 6, 7], [], [(613 * i + 29) % ntok for i in range(100)], [220, 220, 15], [11, ntok, 12]]
    h, hck = bf.load_model(bfutil.model_path("gpt2.i2w")), ck.load("gpt2.i2w")
    handles.append(h)
    want = [ck.ids_to_text(hck, s, 0) for s in seqs]
    ck.free(hck)
    assert want[4] == b"" and want[2]
    out["IdsToTextBatch"] = Form(L.IdsToTextBatch, [VP(h)], [0], seqs, want, ([1, 2, 3, 4, 5, 6, 7], [8, 9, 10]), in_dtype=np.int32)
    # hyphenation: five of the edge words, whose answers the reference gave
    named = wc.edge_words()
    texts = dict(zip([n for n, _ in named], wc.ref_texts("edge", wc.FIXTURE, [w for _, w in named], wc.UHYS)["45"]))
    pick = ["spanish", "empty", "syllables_1_bytes", "space", "long_en"]
    h = bf.load_model(wc.FIXTURE)
    handles.append(h)
    out["WordHyphenationBatch"] = Form(L.WordHyphenationBatch, [VP(h)], [0x2D], [dict(named)[k] for k in pick], [texts[k].encode("latin-1") for k in pick], (b"syllabi", b"fication"))
    # dictionary: a known entry (test_dict_lookup: `pedia`), the empty key, a key of 70 symbols
    keys = [[ord(c) for c in "pedia"], [], [97] * 70, [ord(c) for c in "the"], [ord(c) for c in "zzzzqqq"]]
    dck = sc.DictChecker("gpt2.bin")
    ret, ids, vals, v_off = dck.batch(keys)
    dck.close()
    assert ret[0] > 0
    h = bf.load_model(bfutil.model_path("gpt2.bin"))
    handles.append(h)
    out["DictGetInfoBatch"] = Form(L.DictGetInfoBatch, [VP(h)], [], keys, [vals[v_off[i]:v_off[i + 1]] for i in range(5)], ([ord(c) for c in "xxpedia"], [ord(c) for c in "the"]),
                                   in_dtype=np.int32, out_dtype=np.int32, per_item=(ret, ids))
    yield out
    for h in handles:
        bf.free_model(h)


@pytest.mark.parametrize("name", HOST_FORMS)
def test_first_offset_not_zero_and_null_offsets_out(forms, name):
    f = forms[name]
    r, out, o_off, extra = f.call(f.inside, f.off, f.n, f.T)
    assert np.array_equal(o_off, f.want_off) and o_off[0] == 0
    f.check_output(r, out, extra)
    r, out, o_off, extra = f.call(f.inside, f.off, f.n, f.T, with_off=False)      # NULL offsets_out: the same answer
    f.check_output(r, out, extra)
    assert (o_off == -1).all()


@pytest.mark.parametrize("name", HOST_FORMS)
def test_empty_batch(forms, name):
    f = forms[name]
    r, out, o_off, _ = f.call(None, np.array([5], dtype=np.int64), 0, 0, with_out=False)
    assert r == 0 and o_off.tolist() == [0]
    assert f.call(None, np.array([5], dtype=np.int64), 0, 0, with_out=False, with_off=False)[0] == 0


@pytest.mark.parametrize("name", HOST_FORMS)
def test_null_output_with_a_result(forms, name):
    f = forms[name]
    r, _, o_off, _ = f.call(f.inside, f.off, f.n, f.T, with_out=False)
    assert r == E_ARG
    assert np.array_equal(o_off, f.want_off)


# ---- IdsToRowsBatch: the first offset and the empty batch (it requires row_offsets_out: tests/test_gpu_rows.py)
ROWS = dict(L=8, cls_id=rc.CLS, sep_id=rc.SEP, stride=2, max_rows=0)


def rows_call(h, ids, off, n, cap):
    import blingfire_amd as bf
    L = ROWS["L"]
    rows, mask = np.full(cap * L + 64, CANARY[np.dtype(np.int32)], dtype=np.int32), np.full(cap * L + 64, 0xA5, dtype=np.uint8)
    seq, first = np.full(cap + 64, -77, dtype=np.int32), np.full(cap + 64, -77, dtype=np.int32)
    r_off = np.full(n + 1, -1, dtype=np.int64)
    r = bf.lib().IdsToRowsBatch(VP(h), ptr(ids), ptr(off), n, L, ROWS["cls_id"], ROWS["sep_id"], rc.PAD, ROWS["stride"], ROWS["max_rows"], 0,
                                ptr(rows) if cap else None, ptr(mask) if cap else None, ptr(seq) if cap else None, ptr(first) if cap else None, cap, ptr(r_off))
    return r, (rows, mask, seq, first), r_off


def test_rows_first_offset_not_zero_and_empty_batch():
    import blingfire_amd as bf
    lens = [3, 0, 70, 5, 9]
    off = np.zeros(6, dtype=np.int64)
    np.cumsum(lens, out=off[1:])
    ids = (1000 + np.arange(int(off[-1]))).astype(np.int32)
    want = rc.restate(ids, off, ROWS["L"], ROWS["cls_id"], ROWS["sep_id"], rc.PAD, ROWS["stride"], ROWS["max_rows"])
    total = len(want[2])
    inside = np.ascontiguousarray(np.concatenate([2000 + np.arange(FIRST), ids, 3000 + np.arange(9)]).astype(np.int32))
    h = bf.load_model(bfutil.model_path(bfutil.bert_model_name()))
    try:
        r, got, r_off = rows_call(h, inside, off + FIRST, 5, total)
        assert r == total and np.array_equal(r_off, want[4]) and r_off[0] == 0
        for g, w, width, canary in zip(got, want[:4], (ROWS["L"], ROWS["L"], 1, 1), (CANARY[np.dtype(np.int32)], 0xA5, -77, -77)):
            assert np.array_equal(g[:total * width], w.reshape(-1))
            assert (g[total * width:] == canary).all()
        r, _, r_off = rows_call(h, None, np.array([5], dtype=np.int64), 0, 0)
        assert r == 0 and r_off.tolist() == [0]
    finally:
        bf.free_model(h)
