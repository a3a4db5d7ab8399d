"""Shared TEST catalogue: every call that meets in a handle's device workspaces and its control block (bf_capi.cpp MiscWords), as STEPS that the
GPU tier (tests/test_gpu_call_order.py) runs in every order on one handle and the CPU tier (tests/test_order_host.py) proves fit for that.

A step is a name plus run(h, cx): it makes ONE C-ABI call (the Device calls on torch tensors, the host calls on numpy arrays), synchronises, and
returns (outputs, return value, BfLastStatus behind it).  Its `want` -- every output buffer in full, the return value, the status -- is computed
here, once per process, from what the suite already trusts and never from the library under test: bfutil.reference() / bfutil.oracle() for ids and
byte offsets, the checkers of secondary_cases for words, sentences, ids-to-text and the dictionary, the restatements of rows_cases, pair_cases,
plane_cases, packed_cases, packedplanes_cases, stream_cases, mlm_cases, mlmcap_cases and denoise_cases, the stored answers of w2h_cases.  A step sets the BfSetVariant value it needs (and BfSetHostChunkBytes
where it takes the host path) at its start, so it never depends on what the step before it set, and every output goes into a buffer with TAIL
entries of a sentinel behind its capacity: `want` holds the sentinel there too, so one comparison per buffer covers every element up to the
count, what lies behind it and the offsets in full.

Two batch sizes, both of flat_cases / tiny_cases / bfutil.ADVERSARIAL material:
  big    the smallest batch the default variant sends to the flat program (bf_capi.cpp use_flat: >= 1,024 documents and >= 1 MiB), with handed-back,
         invalid and empty documents;
  small  37 documents of a few KB: below the limits of the mapped host path (256 documents, 64 KiB), no multiple of 64 or 4.
A small step behind a big one of another program finds the big one's entries, lists, counts and spans just past its own extent.

One catalogue per kind of handle (BUILDERS).  wordpiece, unigram and bpe cross the tokenizer programs with the host forms, the secondary calls and
one step of each row stage; i2w crosses IdsToText -- its status 4 included -- with rows, packed rows, MLM, stream rows and a denoise call that
ends with status 1; w2h has hyphenation.  `inputs`, on the WordPiece model again, is the catalogue of the model-input calls, kept apart from
wordpiece because a walk grows with the square of its steps: a Device and a host tokenizer call that feed the others; the packed stage as the
base call, as IdsToPackedRowsPlanesBatchDevice wide and narrow (a NULL plane among its slots) and as its host form; the stream stage, which
borrows the packed stage's widths, block sums and W, with many sequences and few, cut by rows_cap (status 1), with a bad range (status 8) and as
its host form; the host form of the rows-planes call, which owns the plane staging buffers the stream host form puts its labels in; the base MLM
kernel beside RowsMlmPredictionsBatchDevice with max_pred > 0 (the capped kernel) and == 0 (the base kernel again); and RowsDenoiseBatchDevice
with status 0 and with the status 1 its kernel sets by an atomic -- every one of them in front of and behind every other.

The status a step wants is stated where the step is built, with its reason: 0, 1 (bit 0: its capacity was below the need), 8 (bit 3: a range outside
the input) and, for IdsToText alone, 4 (bit 2: a sequence with an unknown id).  Bit 6 (the BPE pool too small) stays out: the pool only grows, so
no step could bring it about again for the step behind it."""
import ctypes

import numpy as np

import bfutil
import blingfire_amd as bf
import denoise_cases
import flat_cases
import mlm_cases
import mlmcap_cases
import packed_cases
import packedplanes_cases
import pair_cases
import plane_cases
import rows_cases
import secondary_cases as sc
import stream_cases
import tiny_cases

VP = ctypes.c_void_p
TAIL = 64
SENTINEL = {np.dtype(np.int32): -7, np.dtype(np.int64): -7, np.dtype(np.uint8): 0x7F}
WP_PAIR, SP_PAIR = (512, 100), (2048, 0)                 # (max_ids_per_doc, unk)
BIG_NHEAD = 1620                                         # flat_cases.mixture(BIG_NHEAD): about 2,200 documents, 1.1 MB
FLAT_MIN_DOCS, FLAT_MIN_BYTES = 1024, 1 << 20            # bf_capi.cpp use_flat
SMALL_MAX_DOCS, SMALL_MAX_BYTES = 256, 64 * 1024         # bf_capi.cpp run_host_locked
LONG_THRESH_MIN, LONG_BYTES_PER_THRESH = 16, 24000       # bf_capi.cpp long_caps
NO_LONG = 0x40000000                                     # bf_variant.h WordsKnobs::no_long
HOST_CHUNK_DEFAULT = 128 << 20                           # bf_capi.cpp Handle::host_chunk_bytes
CLS, SEP, PAD = rows_cases.CLS, rows_cases.SEP, rows_cases.PAD
ROW_LENS = (12, 64)                                      # both span_group slices (a slice of a wave at L <= 32, a whole wave above)

_memo = {}


def memo(key, fn):
    if key not in _memo:
        _memo[key] = fn()
    return _memo[key]


def frozen(*arrays):
    for a in arrays:
        if isinstance(a, np.ndarray):
            a.flags.writeable = False
    return arrays if len(arrays) != 1 else arrays[0]


# ------------------------------------------------------------------------------------------------
# the order: every ordered pair of steps exactly once
# ------------------------------------------------------------------------------------------------
def circuit(n, seed=0):
    """n * n + 1 step numbers in which every ordered pair (a, b) of range(n), a == b included, occurs as neighbours exactly once: an Euler circuit
    of the complete digraph with loops (every vertex has n arcs in and n out), by Hierholzer's algorithm; `seed` rotates the start and the order
    in which a vertex spends its arcs"""
    assert n >= 1
    spent = [0] * n
    stack, out = [seed % n], []
    while stack:
        v = stack[-1]
        if spent[v] < n:
            stack.append((v + seed + spent[v]) % n)
            spent[v] += 1
        else:
            out.append(stack.pop())
    return out[::-1]


# ------------------------------------------------------------------------------------------------
# the two batches
# ------------------------------------------------------------------------------------------------
HANDED_BACK = b"b" * 700 + b" tail"                      # a run of more than flat_cases.WF_RUN_MAX bytes (tests/test_flat_emu.py test_handed_back)
INVALID = b"ab\xff cd"                                   # invalid UTF-8: no ids from a model that decodes


def big_batch():
    def build():
        docs = flat_cases.docs_of(flat_cases.mixture(BIG_NHEAD))
        for k, extra in enumerate((HANDED_BACK, b"with [UNK] inside", INVALID, b"", b"\x80abc")):
            docs.insert(len(docs) * (k + 1) // 6, extra)
        return frozen(*flat_cases.pack(docs))
    return memo("big", build)


def small_docs():
    edge = {n: (fill * (n // len(fill) + 1))[:n] for n, fill in ((63, b"a "), (64, b"ab, "), (65, "é ".encode()), (513, b"word "))}
    docs = list(bfutil.ADVERSARIAL[:18]) + [b"", b""] + list(tiny_cases.SPECIALS) + [edge[63], edge[64], edge[65], edge[513], b"word " * 200,
                                                                                     b"the last document has an answer"]
    assert len(docs) == 37
    return docs


def small_batch():
    return memo("small", lambda: frozen(*flat_cases.pack(small_docs())))


def batch(size):
    return big_batch() if size == "big" else small_batch()


def empty_batch():
    return memo("empty", lambda: frozen(np.zeros(0, dtype=np.uint8), np.zeros(1, dtype=np.int64)))


def bad_range_offsets(off):
    """the offsets with the last document claiming 1,000 bytes behind the text (tests/test_gpu_api.py): that document is empty, bit 3"""
    bad = off.copy()
    bad[-1] += 1000
    return frozen(bad)


# ------------------------------------------------------------------------------------------------
# the checkers' answers
# ------------------------------------------------------------------------------------------------
OFFSETS_NAME = "TextToIdsWithOffsets" if bfutil.have_ref() else "bfo_text_to_ids_with_offsets"


def t2i_checker(model):
    def load():
        ck = bfutil.reference() if bfutil.have_ref() else bfutil.oracle()
        return ck, ck.load(bfutil.model_path(model))
    return memo(("t2i checker", model), load)


def ids_answer(model, size, pair, drop_last=False):
    """(ids, None, None, id offsets) of the checker's TextToIds for every document; drop_last: the last document counts as empty"""
    def compute():
        text, off = batch(size)
        _, ids, ido = bfutil.cpu_ids_compact(bfutil.checker_lib_path()[0], bfutil.model_path(model), text, off, pair[0], pair[1])
        return frozen(ids.astype(np.int32), None, None, ido)
    ids, _, _, ido = memo(("ids", model, size, pair), compute)
    if drop_last:
        ido2 = ido.copy()
        ido2[-1] = ido2[-2]
        return frozen(ids[:ido2[-1]], None, None, ido2)
    return ids, None, None, ido


def offsets_answer(model, size, pair):
    """(ids, first bytes, last bytes, id offsets) of the checker's TextToIdsWithOffsets, one document at a time; its ids equal ids_answer's"""
    def compute():
        ck, hck = t2i_checker(model)
        text, off = batch(size)
        raw = text.tobytes()
        wi, ws, we = [], [], []
        ido = np.zeros(len(off), dtype=np.int64)
        for d in range(len(off) - 1):
            b = raw[off[d]:off[d + 1]]
            c, i_, s_, e_ = ck.with_offsets(hck, b, min(pair[0], 2 * len(b) + 2), pair[1], OFFSETS_NAME)
            wi += i_; ws += s_; we += e_
            ido[d + 1] = ido[d] + c
        out = frozen(np.array(wi, dtype=np.int32), np.array(ws, dtype=np.int32), np.array(we, dtype=np.int32), ido)
        ids, _, _, ido0 = ids_answer(model, size, pair)
        assert np.array_equal(ido, ido0) and np.array_equal(out[0], ids), "the checker's TextToIdsWithOffsets and TextToIds disagree"
        return out
    return memo(("offsets", model, size, pair), compute)


# ------------------------------------------------------------------------------------------------
# steps
# ------------------------------------------------------------------------------------------------
class Want:
    """one output buffer as it must be, in full.  where: how a difference is named -- ("docs", offsets) an element of a ragged array,
    ("rows", L) a cell of a row, ("items",) an entry per document, row or sequence"""

    def __init__(self, label, array, where=("items",)):
        self.label, self.array, self.where = label, frozen(np.ascontiguousarray(array)), where


class Step:
    def __init__(self, name, call, want, ret=0, status=0, why="", size="small", after=None):
        self.name, self.call, self.want, self.ret, self.status, self.why, self.size, self.after = name, call, want, ret, status, why, size, after

    def run(self, h, cx):
        """-> (outputs in the order of self.want, the return value, the BfLastStatus read behind the call)"""
        ret, outs = self.call(h, cx)
        cx.synchronize()
        return outs, ret, bf.lib().BfLastStatus(VP(h))


class Context:
    """the GPU tier's side of a step: the device, the stream, uploads that are made once and kept, sentinel-filled output tensors"""

    def __init__(self):
        import torch
        self.torch = torch
        self.dev = torch.device("cuda", 0)
        self.stream = VP(torch.cuda.current_stream(self.dev).cuda_stream)
        self._up = {}

    def up(self, a):
        """the device copy of an input (or wanted) array, made once; an array without elements is a 1-element dummy allocation"""
        if id(a) not in self._up:
            src = a if a.size else np.zeros(1, dtype=a.dtype)
            self._up[id(a)] = (a, self.torch.from_numpy(np.array(src)).to(self.dev))
        return self._up[id(a)][1]

    def ptr(self, a):
        return self.up(a).data_ptr()

    def full(self, n, dtype):
        dtype = np.dtype(dtype)
        return self.torch.full((max(n, 1),), SENTINEL[dtype], dtype=getattr(self.torch, dtype.name), device=self.dev)

    def synchronize(self):
        self.torch.cuda.synchronize(self.dev)


def padded(a, cap, dtype=None):
    """the first min(cap, len) elements of `a` and the sentinel up to cap + TAIL entries: a whole output buffer as it must be"""
    a = np.asarray(a).reshape(-1)
    dtype = np.dtype(dtype or a.dtype)
    n = min(cap, len(a))
    return np.concatenate([a[:n].astype(dtype), np.full(max(cap + TAIL, 1) - n, SENTINEL[dtype], dtype=dtype)])


def set_variant(h, variant):
    assert bf.lib().BfSetVariant(VP(h), variant) >= 0, "BfSetVariant refused %#x" % variant


def set_host_chunk(h, nbytes):
    f = bf.lib().BfSetHostChunkBytes
    f.restype, f.argtypes = ctypes.c_int64, [VP, ctypes.c_int64]
    assert f(VP(h), nbytes) >= 0


def tok_device_step(name, size, inputs, ans, variant, pair, cap=None, status=0, why="status 0: ids_cap is the exact total, every range inside the text"):
    """TextToIdsBatchDevice, or TextToIdsWithOffsetsBatchDevice when `ans` carries byte offsets, with ids_cap == cap (default: the exact total)"""
    text, off = inputs
    ids, st, en, ido = ans
    nd, with_off = len(off) - 1, st is not None
    cap = int(ido[-1]) if cap is None else cap
    where = ("docs", ido)
    want = [Want("ids", padded(ids, cap), where)] + ([Want("first bytes", padded(st, cap), where), Want("last bytes", padded(en, cap), where)] if with_off else [])
    want.append(Want("id offsets", ido))

    def call(h, cx):
        set_variant(h, variant)
        outs = [cx.full(cap + TAIL, np.int32) for _ in range(3 if with_off else 1)]
        o = cx.full(nd + 1, np.int64)
        L = bf.lib()
        if with_off:
            r = L.TextToIdsWithOffsetsBatchDevice(VP(h), cx.ptr(text), cx.ptr(off), nd, len(text), outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), cap,
                                                  o.data_ptr(), pair[0], pair[1], cx.stream)
        else:
            r = L.TextToIdsBatchDevice(VP(h), cx.ptr(text), cx.ptr(off), nd, len(text), outs[0].data_ptr(), cap, o.data_ptr(), pair[0], pair[1], cx.stream)
        return r, outs + [o]
    return Step(name, call, want, 0, status, why, size)


def host_batch_step(name, size, ans, variant, pair, chunk=HOST_CHUNK_DEFAULT, why="status 0: the capacity is the exact total"):
    """TextToIdsBatch on host arrays; returns the id total"""
    text, off = batch(size)
    ids, _, _, ido = ans
    nd, total = len(off) - 1, int(ido[-1])
    want = [Want("ids", padded(ids, total), ("docs", ido)), Want("id offsets", ido)]

    def call(h, cx):
        set_variant(h, variant)
        set_host_chunk(h, chunk)
        out, o = np.full(total + TAIL, -7, dtype=np.int32), np.full(nd + 1, -7, dtype=np.int64)
        r = bf.lib().TextToIdsBatch(VP(h), text.ctypes.data, off.ctypes.data, nd, out.ctypes.data, total, o.ctypes.data, pair[0], pair[1])
        return r, [out, o]
    return Step(name, call, want, total, 0, why, size)


def host_single_step(name, model, doc, pair, with_off):
    """TextToIds / TextToIdsWithOffsets of one document: what is written ends at the count, the rest of the arrays stays as it was"""
    ck, hck = t2i_checker(model)
    mx, unk = pair
    if with_off:
        c, i_, s_, e_ = ck.with_offsets(hck, doc, mx, unk, OFFSETS_NAME)
        want = [Want(w, padded(np.array(a, dtype=np.int32), mx)) for w, a in (("ids", i_), ("first bytes", s_), ("last bytes", e_))]
    else:
        c, buf = ck.text_to_ids(hck, doc, mx, unk)
        want = [Want("ids", padded(np.array(buf[:min(c, mx)], dtype=np.int32), mx))]
    assert 0 < c <= mx

    def call(h, cx):
        set_variant(h, 3)
        outs = [np.full(mx + TAIL, -7, dtype=np.int32) for _ in want]
        if with_off:
            r = bf.lib().TextToIdsWithOffsets(VP(h), doc, len(doc), outs[0].ctypes.data, outs[1].ctypes.data, outs[2].ctypes.data, mx, unk)
        else:
            r = bf.lib().TextToIds(VP(h), doc, len(doc), outs[0].ctypes.data, mx, unk)
        return r, outs
    return Step(name, call, want, c, 0, "status 0: one document, all of its ids fit")


def long_threshold(total_bytes):
    return max(LONG_THRESH_MIN, total_bytes // LONG_BYTES_PER_THRESH)


def words_step(name, size, model, mode, variant):
    """TextToWordsBatchDevice (mode 1) / TextToSentencesBatchDevice (mode 2) on the tokenizer's own handle, text_cap == the exact total"""
    text, off = batch(size)
    nd = len(off) - 1

    def compute():
        ck = memo("secondary checker", sc.Checker)
        hck = memo(("secondary model", model), lambda: ck.load(model))
        raw = text.tobytes()
        fn = ck.words if mode == 1 else ck.sentences
        return frozen(*sc.pack([fn(raw[off[d]:off[d + 1]], hck) for d in range(nd)]))
    w_text, w_off = memo(("words", model, size, mode), compute)
    total = int(w_off[-1])
    want = [Want("text", padded(w_text, total), ("docs", w_off)), Want("text offsets", w_off)]

    def call(h, cx):
        set_variant(h, variant)
        out, o = cx.full(total + TAIL, np.uint8), cx.full(nd + 1, np.int64)
        fn = bf.lib().TextToWordsBatchDevice if mode == 1 else bf.lib().TextToSentencesBatchDevice
        return fn(VP(h), cx.ptr(text), cx.ptr(off), nd, len(text), out.data_ptr(), total, o.data_ptr(), cx.stream), [out, o]
    return Step(name, call, want, 0, 0, "status 0: text_cap is the exact total, every range inside the text", size)


# ---- the row stage and the calls behind it: their ids are the checker's, uploaded once
def row_geometry_ok(ido, L, cls_id=CLS, sep_id=SEP):
    """the condition of every row-stage step: a sequence of more ids than a row's body (more than one window) and an empty sequence"""
    body = L - (cls_id >= 0) - (sep_id >= 0)
    n = np.diff(ido)
    return bool((n > body).any() and (n == 0).any())


def rows_step(name, size, ids, ido, L, stride, max_rows, planes=None, narrow=False):
    """IdsToRowsBatchDevice, or IdsToRowsPlanesBatchDevice with planes = (sources, fills), rows_cap == the exact total.  Both L of ROW_LENS are
    multiples of 4, so aligned outputs take the wide stores (W == 4); narrow: d_rows_out begins 4 bytes behind a 16-byte boundary, one sentinel
    entry into its buffer, and the fill stores cell by cell (W == 1)"""
    nseq = len(ido) - 1
    rows, mask, seq, first, r_off, status = rows_cases.restate(ids, ido, L, CLS, SEP, PAD, stride, max_rows)
    assert status == 0
    R = len(seq)
    lead = 1 if narrow else 0
    want = [Want("rows", np.concatenate([np.full(lead, -7, dtype=np.int32), padded(rows, R * L)]), ("rows", L, lead)), Want("mask", padded(mask, R * L), ("rows", L)), Want("row_seq", padded(seq, R)), Want("row_first", padded(first, R)),
            Want("row offsets", r_off)]
    src, fill = planes if planes else ((), ())
    if planes:
        w_planes, seq2, first2, r_off2, status = plane_cases.restate_planes(ido, L, CLS, SEP, stride, max_rows, False, src, fill, ids_len=len(ids))
        assert status == 0 and np.array_equal(r_off2, r_off) and np.array_equal(seq2, seq)
        want += [Want("plane %d" % k, padded(p, R * L), ("rows", L)) for k, p in enumerate(w_planes)]

    def call(h, cx):
        outs = [cx.full(lead + R * L + TAIL, np.int32), cx.full(R * L + TAIL, np.uint8), cx.full(R + TAIL, np.int32), cx.full(R + TAIL, np.int32), cx.full(nseq + 1, np.int64)]
        assert outs[0].data_ptr() % 16 == 0
        pre = (VP(h), cx.ptr(ids), len(ids), cx.ptr(ido), nseq, L, CLS, SEP, PAD, stride, max_rows, 0, outs[0].data_ptr() + 4 * lead, *[o.data_ptr() for o in outs[1:4]], R,
               outs[4].data_ptr())
        if not planes:
            return bf.lib().IdsToRowsBatchDevice(*pre, cx.stream), outs
        pl = [cx.full(R * L + TAIL, np.int32) for _ in src]
        c_src = (VP * len(src))(*[cx.ptr(s) for s in src])
        c_fill = (ctypes.c_int32 * len(src))(*fill)
        c_out = (VP * len(src))(*[p.data_ptr() for p in pl])
        return bf.lib().IdsToRowsPlanesBatchDevice(*pre, len(src), c_src, c_fill, c_out, cx.stream), outs + pl
    return Step(name, call, want, 0, 0, "status 0: every id range inside [0, ids_len], rows_cap is the exact total", size)


def pair_rows_step(name, size, ids, ido, L, max_a, stride):
    """IdsToPairRowsBatchDevice, the QA form (mode 0, every window): the question of pair q is sequence q, its context sequence (q + 1) % nseq of
    the same id array"""
    nseq = len(ido) - 1
    order = (np.arange(nseq) + 1) % nseq
    ids_b, off_b = sc.tile(ids, ido, order)
    frozen(ids_b, off_b)
    rows, mask, typ, seq, first, r_off, status = pair_cases.restate(ids, ido, ids_b, off_b, L, CLS, SEP, PAD, 0, max_a, stride, 0)
    assert status == 0
    R = len(seq)
    want = [Want("rows", padded(rows, R * L), ("rows", L)), Want("mask", padded(mask, R * L), ("rows", L)), Want("type", padded(typ, R * L), ("rows", L)),
            Want("row_seq", padded(seq, R)), Want("row_first_b", padded(first, R)), Want("row offsets", r_off)]

    def call(h, cx):
        outs = [cx.full(R * L + TAIL, np.int32), cx.full(R * L + TAIL, np.uint8), cx.full(R * L + TAIL, np.uint8), cx.full(R + TAIL, np.int32), cx.full(R + TAIL, np.int32),
                cx.full(nseq + 1, np.int64)]
        r = bf.lib().IdsToPairRowsBatchDevice(VP(h), cx.ptr(ids), len(ids), cx.ptr(ido), cx.ptr(ids_b), len(ids_b), cx.ptr(off_b), nseq, L, CLS, SEP, PAD, 0, max_a, stride, 0, 0,
                                              *[o.data_ptr() for o in outs[:5]], R, outs[5].data_ptr(), cx.stream)
        return r, outs
    step = Step(name, call, want, 0, 0, "status 0: every id range of both sides inside its array, rows_cap is the exact total", size)
    step.off_b = off_b
    return step


def packed_step(name, size, ids, ido, L):
    """IdsToPackedRowsBatchDevice with rows_cap == R"""
    nseq = len(ido) - 1
    rows, seg, pos, first, seq_row, seq_col, R, status = packed_cases.restate(ids, ido, L, CLS, SEP, PAD, rows_cap=None)
    assert status == 0
    want = [Want(w, padded(a, R * L), ("rows", L)) for w, a in (("rows", rows), ("seg", seg), ("pos", pos))]
    want += [Want("row_first_seq", padded(first, R + 1)), Want("seq_row", padded(seq_row, nseq)), Want("seq_col", padded(seq_col, nseq)),
             Want("nrows", padded(np.array([R], dtype=np.int64), 1))]

    def call(h, cx):
        outs = [cx.full(R * L + TAIL, np.int32) for _ in range(3)] + [cx.full(R + 1 + TAIL, np.int32), cx.full(nseq + TAIL, np.int32), cx.full(nseq + TAIL, np.int32),
                                                                       cx.full(1 + TAIL, np.int64)]
        r = bf.lib().IdsToPackedRowsBatchDevice(VP(h), cx.ptr(ids), len(ids), cx.ptr(ido), nseq, L, CLS, SEP, PAD, 0, *[o.data_ptr() for o in outs[:4]], R,
                                                *[o.data_ptr() for o in outs[4:]], cx.stream)
        return r, outs
    return Step(name, call, want, 0, 0, "status 0: every id range inside [0, ids_len], rows_cap is R", size)


def row_planes(ids, ido, st, en, L, stride, max_rows):
    """(rows, mask, row_seq, first-byte plane, last-byte plane) of the restatements: the inputs of the span-cell and MLM steps"""
    rows, mask, seq, _, _, status = rows_cases.restate(ids, ido, L, CLS, SEP, PAD, stride, max_rows)
    (S, E), _, _, _, status2 = plane_cases.restate_planes(ido, L, CLS, SEP, stride, max_rows, False, (st, en), (-1, -1), ids_len=len(ids))
    assert status == 0 and status2 == 0
    return frozen(rows, mask, seq, S, E)


def span_step(name, size, ids, ido, st, en, L):
    """RowsSpanCellsBatchDevice over the offset planes of every window of every document; the span of document q is bytes [3 + q % 5, 11 + q % 7],
    of every ninth document nothing (a = -1)"""
    nseq = len(ido) - 1
    _, _, seq, S, E = row_planes(ids, ido, st, en, L, 2, 0)
    q = np.arange(nseq)
    a, z = (3 + q % 5).astype(np.int32), (11 + q % 7).astype(np.int32)
    a[::9] = -1
    frozen(a, z)
    start, end, status = plane_cases.restate_span(S, E, seq, nseq, a, z, 0)
    assert status == 0
    R = len(seq)
    want = [Want("start cells", padded(start, R)), Want("end cells", padded(end, R))]

    def call(h, cx):
        outs = [cx.full(R + TAIL, np.int32) for _ in range(2)]
        r = bf.lib().RowsSpanCellsBatchDevice(VP(h), cx.ptr(S), cx.ptr(E), L, R, None, cx.ptr(seq), nseq, cx.ptr(a), cx.ptr(z), 0, outs[0].data_ptr(), outs[1].data_ptr(), cx.stream)
        return r, outs
    return Step(name, call, want, 0, 0, "status 0: every row's item is inside [0, nseq)", size)


MLM_SEED, MLM_EPOCH = 0x1234567887654321, 3


def mlm_step(name, size, ids, ido, st, en, L):
    """RowsMlmMaskBatchDevice over every window of every document; with byte-offset planes (st, en) it masks whole words, without them cells"""
    whole = st is not None
    if whole:
        rows, mask, _, S, E = row_planes(ids, ido, st, en, L, 2, 0)
    else:
        rows, mask = frozen(*rows_cases.restate(ids, ido, L, CLS, SEP, PAD, 2, 0)[:2])
        S = E = None
    R = len(rows)
    specials = (CLS, SEP, PAD)
    w_ids, w_labels = mlm_cases.restate_mlm(rows, mask, None, S, E, specials, mlm_cases.DEFAULT_PROBS, mlm_cases.MASK, mlm_cases.RAND_RANGE, -100, MLM_SEED, MLM_EPOCH,
                                            heads_fn=mlm_cases.heads_array)
    want = [Want("masked ids", padded(w_ids, R * L), ("rows", L)), Want("labels", padded(w_labels, R * L), ("rows", L))]

    def call(h, cx):
        outs = [cx.full(R * L + TAIL, np.int32) for _ in range(2)]
        c_spec = (ctypes.c_int32 * len(specials))(*specials)
        r = bf.lib().RowsMlmMaskBatchDevice(VP(h), cx.ptr(rows), L, R, None, cx.ptr(mask), None, cx.ptr(S) if whole else None, cx.ptr(E) if whole else None, len(specials), c_spec,
                                            *mlm_cases.DEFAULT_PROBS, mlm_cases.MASK, *mlm_cases.RAND_RANGE, -100, MLM_SEED, MLM_EPOCH, outs[0].data_ptr(), outs[1].data_ptr(),
                                            cx.stream)
        return r, outs
    return Step(name, call, want, 0, 0, "status 0: the call sets no bit", size)


# ---- the model-input calls: packed planes, stream rows, capped MLM, span corruption, and the host-buffer forms of the row stages
IGN = stream_cases.IGN
BEHIND_ROWS = 3                                          # rows behind *d_nrows in the inputs and outputs of the denoise steps: never read, never written
PRED_CAP = 2                                             # max_pred of the predictions step: tests/test_order_host.py proves that it binds in some rows and not in others
DENOISE_TRUNCATED_DEC = 3                                # dec_len of the truncated denoise steps: a row with a span loses cells, a row without one (eos alone) does not


def host_buffers(caps):
    """sentinel-filled numpy outputs of a host-buffer call, one per (entries, dtype) with TAIL entries behind it"""
    return [np.full(max(n + TAIL, 1), SENTINEL[np.dtype(t)], dtype=t) for n, t in caps]


def packed_answer(ids, ido, L):
    """packed_cases.restate with rows_cap == R, once per (ids, L); the status is 0"""
    def compute():
        out = packed_cases.restate(ids, ido, L, CLS, SEP, PAD, rows_cap=None)
        assert out[7] == 0
        return (ids, ido), frozen(*out[:6]) + (out[6],)                # (the key holds ids of objects: the entry keeps them alive)
    return memo(("packed answer", id(ids), id(ido), L), compute)[1]


def packed_wants(ids, ido, L, with_nrows):
    rows, seg, pos, first, seq_row, seq_col, R = packed_answer(ids, ido, L)
    nseq = len(ido) - 1
    want = [Want(w, padded(a, R * L), ("rows", L)) for w, a in (("packed rows", rows), ("seg", seg), ("pos", pos))]
    want += [Want("row_first_seq", padded(first, R + 1)), Want("seq_row", padded(seq_row, nseq)), Want("seq_col", padded(seq_col, nseq))]
    if with_nrows:
        want.append(Want("nrows", padded(np.array([R], dtype=np.int64), 1)))
    return want, R


def packed_planes_step(name, size, ids, ido, L, src, fill, narrow=False, skip_last=False):
    """IdsToPackedRowsPlanesBatchDevice with rows_cap == R and one plane per source.  narrow: plane 0 begins 4 bytes behind a 16-byte boundary, one
    sentinel entry into its buffer (as rows_step(narrow=True)), so every plane is stored cell by cell; skip_last: the last plane's out is NULL"""
    nseq = len(ido) - 1
    want, R = packed_wants(ids, ido, L, True)
    planes = packedplanes_cases.restate_packed_planes(ido, L, CLS, SEP, src, fill, ids_len=len(ids))
    taken = len(src) - (1 if skip_last else 0)
    lead = 1 if narrow else 0
    for k in range(taken):
        front = np.full(lead if k == 0 else 0, -7, dtype=np.int32)
        want.append(Want("plane %d" % k, np.concatenate([front, padded(planes[k], R * L)]), ("rows", L, len(front))))

    def call(h, cx):
        outs = [cx.full(R * L + TAIL, np.int32) for _ in range(3)] + [cx.full(R + 1 + TAIL, np.int32), cx.full(nseq + TAIL, np.int32), cx.full(nseq + TAIL, np.int32),
                                                                       cx.full(1 + TAIL, np.int64)]
        pl = [cx.full((lead if k == 0 else 0) + R * L + TAIL, np.int32) for k in range(taken)]
        ptrs = [p.data_ptr() + (4 * lead if k == 0 else 0) for k, p in enumerate(pl)]
        assert all(p.data_ptr() % 16 == 0 for p in pl) and (not narrow or ptrs[0] % 16 == 4)
        c_src = (VP * len(src))(*[cx.ptr(s) for s in src])
        c_fill = (ctypes.c_int32 * len(src))(*fill)
        c_out = (VP * len(src))(*(ptrs + [None] * (len(src) - taken)))
        r = bf.lib().IdsToPackedRowsPlanesBatchDevice(VP(h), cx.ptr(ids), len(ids), cx.ptr(ido), nseq, L, CLS, SEP, PAD, 0, *[o.data_ptr() for o in outs[:4]], R,
                                                      *[o.data_ptr() for o in outs[4:]], len(src), c_src, c_fill, c_out, cx.stream)
        return r, outs + pl
    step = Step(name, call, want, 0, 0, "status 0: every id range inside [0, ids_len], rows_cap is R", size)
    step.L, step.fill, step.taken, step.plane_lead = L, tuple(fill), taken, lead
    return step


def packed_planes_host_step(name, size, ids, ido, L, src, fill):
    """IdsToPackedRowsPlanesBatch into numpy buffers with rows_cap == R; returns R"""
    nseq = len(ido) - 1
    want, R = packed_wants(ids, ido, L, False)
    planes = packedplanes_cases.restate_packed_planes(ido, L, CLS, SEP, src, fill)
    want += [Want("plane %d" % k, padded(p, R * L), ("rows", L)) for k, p in enumerate(planes)]

    def call(h, cx):
        outs = host_buffers([(R * L, np.int32)] * 3 + [(R + 1, np.int32), (nseq, np.int32), (nseq, np.int32)] + [(R * L, np.int32)] * len(src))
        c_src = (VP * len(src))(*[s.ctypes.data for s in src])
        c_fill = (ctypes.c_int32 * len(src))(*fill)
        c_out = (VP * len(src))(*[o.ctypes.data for o in outs[6:]])
        r = bf.lib().IdsToPackedRowsPlanesBatch(VP(h), ids.ctypes.data, ido.ctypes.data, nseq, L, CLS, SEP, PAD, 0, *[o.ctypes.data for o in outs[:4]], R,
                                                outs[4].ctypes.data, outs[5].ctypes.data, len(src), c_src, c_fill, c_out)
        return r, outs
    step = Step(name, call, want, R, 0, "status 0: every id range inside the ids, rows_cap is R", size)
    step.L, step.fill, step.taken, step.plane_lead = L, tuple(fill), len(src), 0
    return step


def rows_planes_host_step(name, size, ids, ido, L, stride, max_rows, src, fill):
    """IdsToRowsPlanesBatch into numpy buffers with rows_cap == the exact total; returns the total"""
    nseq = len(ido) - 1
    rows, mask, seq, first, r_off, status = rows_cases.restate(ids, ido, L, CLS, SEP, PAD, stride, max_rows)
    w_planes, seq2, _, r_off2, status2 = plane_cases.restate_planes(ido, L, CLS, SEP, stride, max_rows, False, src, fill, ids_len=len(ids))
    assert status == 0 and status2 == 0 and np.array_equal(r_off2, r_off) and np.array_equal(seq2, seq)
    R = len(seq)
    want = [Want("rows", padded(rows, R * L), ("rows", L)), Want("mask", padded(mask, R * L), ("rows", L)), Want("row_seq", padded(seq, R)), Want("row_first", padded(first, R)),
            Want("row offsets", r_off)]
    want += [Want("plane %d" % k, padded(p, R * L), ("rows", L)) for k, p in enumerate(w_planes)]

    def call(h, cx):
        outs = host_buffers([(R * L, np.int32), (R * L, np.uint8), (R, np.int32), (R, np.int32)]) + [np.full(nseq + 1, -7, dtype=np.int64)]
        pl = host_buffers([(R * L, np.int32)] * len(src))
        c_src = (VP * len(src))(*[s.ctypes.data for s in src])
        c_fill = (ctypes.c_int32 * len(src))(*fill)
        c_out = (VP * len(src))(*[p.ctypes.data for p in pl])
        r = bf.lib().IdsToRowsPlanesBatch(VP(h), ids.ctypes.data, ido.ctypes.data, nseq, L, CLS, SEP, PAD, stride, max_rows, 0, *[o.ctypes.data for o in outs[:4]], R,
                                          outs[4].ctypes.data, len(src), c_src, c_fill, c_out)
        return r, outs + pl
    return Step(name, call, want, R, 0, "status 0: every id range inside the ids, rows_cap is the exact total", size)


def stream_answer(ids, off, L, bos, eos, flags, ids_len=None):
    """stream_cases.restate_np, once per input: tests/test_order_host.py holds it to the sequential stream_cases.restate on every small step"""
    return memo(("stream answer", id(ids), id(off), L, bos, eos, flags, ids_len),
                lambda: ((ids, off), stream_cases.restate_np(ids, off, L, bos, eos, PAD, IGN, flags, ids_len=len(ids) if ids_len is None else ids_len)))[1]


def stream_step(name, size, ids, off, L, bos, eos, flags=0, rows_cap=None, host=False, status=0, why="status 0: every id range inside [0, ids_len], rows_cap is R"):
    """IdsToStreamRowsBatchDevice with all eight outputs and d_nrows_out = {R, T}, or (host) IdsToStreamRowsBatch into numpy buffers, which returns R;
    rows_cap None = R.  Nothing at or past rows_cap of a row output is written: `want` holds the sentinel there"""
    nseq = len(off) - 1
    ans = stream_answer(ids, off, L, bos, eos, flags)
    R, T = ans[8], ans[9]
    cap = R if rows_cap is None else rows_cap
    assert status == (ans[10] | (1 if R > cap else 0)) and not (host and status)
    want = [Want("stream " + w, padded(a, cap * L), ("rows", L)) for w, a in zip(stream_cases.NAMES[:4], ans[:4])]
    want += [Want(w, padded(a, cap)) for w, a in zip(stream_cases.NAMES[4:6], ans[4:6])] + [Want(w, padded(a, nseq)) for w, a in zip(stream_cases.NAMES[6:], ans[6:8])]
    caps = [(cap * L, np.int32)] * 4 + [(cap, np.int32)] * 2 + [(nseq, np.int32)] * 2
    if not host:
        want.append(Want("nrows", padded(np.array([R, T], dtype=np.int64), 2)))

    def call_device(h, cx):
        outs = [cx.full(n + TAIL, t) for n, t in caps] + [cx.full(2 + TAIL, np.int64)]
        r = bf.lib().IdsToStreamRowsBatchDevice(VP(h), cx.ptr(ids), len(ids), cx.ptr(off), nseq, L, bos, eos, PAD, IGN, flags, *[o.data_ptr() for o in outs[:6]], cap,
                                                *[o.data_ptr() for o in outs[6:]], cx.stream)
        return r, outs

    def call_host(h, cx):
        outs = host_buffers(caps)
        r = bf.lib().IdsToStreamRowsBatch(VP(h), ids.ctypes.data, off.ctypes.data, nseq, L, bos, eos, PAD, IGN, flags, *[o.ctypes.data for o in outs[:6]], cap,
                                          outs[6].ctypes.data, outs[7].ctypes.data)
        return r, outs
    step = Step(name, call_host if host else call_device, want, R if host else 0, status, why, size)
    step.stream = dict(ids=ids, off=off, L=L, bos=bos, eos=eos, flags=flags, rows_cap=cap, R=R, T=T)
    return step


def stream_rows(ids, ido, L, bos=CLS, eos=SEP):
    """(rows, seg) of the restated stream rows, flags 0: the inputs of the denoise steps"""
    ans = stream_answer(ids, ido, L, bos, eos, 0)
    return ans[0], ans[1]


def packed_mlm_inputs(ids, ido, st, en, L):
    """(rows, seg, first-byte plane, last-byte plane) of the restated packed rows: the inputs of the predictions steps"""
    def compute():
        rows, seg = packed_answer(ids, ido, L)[:2]
        S, E = packedplanes_cases.restate_packed_planes(ido, L, CLS, SEP, (st, en), (-1, -1), ids_len=len(ids))
        return (ids, ido), frozen(rows, seg, S, E)
    return memo(("packed mlm inputs", id(ids), id(ido), L), compute)[1]


MLM_SPECIALS = (CLS, SEP, PAD)


def predictions_step(name, size, ids, ido, st, en, L, max_pred):
    """RowsMlmPredictionsBatchDevice over the packed rows with their segment plane and the two byte-offset planes (whole words).  max_pred > 0: all
    five outputs (k_rows_mlm_cap); max_pred == 0: the gathered outputs NULL, the base kernel, and `want` is mlm_cases.restate_mlm's"""
    rows, seg, S, E = packed_mlm_inputs(ids, ido, st, en, L)
    R = len(rows)
    kw = dict(special_ids=MLM_SPECIALS, probs=mlmcap_cases.PROBS, mask_id=mlm_cases.MASK, rand_range=mlm_cases.RAND_RANGE, ignore_label=-100, seed=MLM_SEED, epoch=MLM_EPOCH)
    if max_pred:
        w = mlmcap_cases.restate_cap(rows, None, seg, S, E, max_pred=max_pred, **kw)
        want = [Want("masked ids", padded(w[0], R * L), ("rows", L)), Want("labels", padded(w[1], R * L), ("rows", L)), Want("prediction cells", padded(w[2], R * max_pred), ("rows", max_pred)),
                Want("prediction labels", padded(w[3], R * max_pred), ("rows", max_pred)), Want("prediction count", padded(w[4], R))]
    else:
        w = mlm_cases.restate_mlm(rows, None, seg, S, E, **kw)
        want = [Want("masked ids", padded(w[0], R * L), ("rows", L)), Want("labels", padded(w[1], R * L), ("rows", L))]

    def call(h, cx):
        outs = [cx.full(R * L + TAIL, np.int32) for _ in range(2)] + ([cx.full(R * max_pred + TAIL, np.int32), cx.full(R * max_pred + TAIL, np.int32), cx.full(R + TAIL, np.int32)] if max_pred else [])
        c_spec = (ctypes.c_int32 * len(MLM_SPECIALS))(*MLM_SPECIALS)
        gathered = [o.data_ptr() for o in outs[2:]] if max_pred else [None] * 3
        r = bf.lib().RowsMlmPredictionsBatchDevice(VP(h), cx.ptr(rows), L, R, None, None, cx.ptr(seg), cx.ptr(S), cx.ptr(E), len(MLM_SPECIALS), c_spec, *mlmcap_cases.PROBS,
                                                   mlm_cases.MASK, *mlm_cases.RAND_RANGE, -100, MLM_SEED, MLM_EPOCH, outs[0].data_ptr(), outs[1].data_ptr(), max_pred, *gathered, cx.stream)
        return r, outs
    step = Step(name, call, want, 0, 0, "status 0: the call sets no bit", size)
    step.mlm = dict(rows=rows, seg=seg, S=S, E=E, max_pred=max_pred, kw=kw)
    return step


def denoise_spec():
    """the case table's defaults (denoise_cases.DEFAULTS with the T5 sentinels) over rows of this model: [SEP] closes a sequence, so it is the eos, and
    with [CLS] and the padding it is special -- no span crosses it"""
    return dict(denoise_cases.DEFAULTS, special_ids=MLM_SPECIALS, eos_id=SEP, pad_id=PAD)


def denoise_step(name, size, rows, seg, L, enc_len, dec_len, status, why):
    """RowsDenoiseBatchDevice over R rows and their segment plane with rows_cap = R + BEHIND_ROWS and *d_nrows = R: the rows behind the bound hold
    eligible cells in the input (if the call looked at them) and keep the sentinel in all seven outputs"""
    R = len(rows)
    cap = R + BEHIND_ROWS
    spec = denoise_spec()
    w = denoise_cases.restate_denoise(rows, None, seg, enc_len=enc_len, dec_len=dec_len, **spec)
    assert w["status"] == status
    width = dict(enc=enc_len, enc_cell=enc_len, dec=dec_len, dec_cell=dec_len, enc_count=1, dec_count=1, span_count=1)
    want = [Want(n, padded(w[n], cap * width[n]), ("rows", width[n]) if width[n] > 1 else ("items",)) for n in denoise_cases.NAMES]
    rows_in = frozen(np.concatenate([rows.reshape(-1), np.full(BEHIND_ROWS * L, 4242, dtype=np.int32)]))
    seg_in = frozen(np.concatenate([seg.reshape(-1), np.ones(BEHIND_ROWS * L, dtype=np.int32)]))
    nrows = frozen(np.array([R], dtype=np.int64))

    def call(h, cx):
        outs = [cx.full(cap * width[n] + TAIL, np.int32) for n in denoise_cases.NAMES]
        c_spec = (ctypes.c_int32 * len(spec["special_ids"]))(*spec["special_ids"])
        o = [t.data_ptr() for t in outs]
        r = bf.lib().RowsDenoiseBatchDevice(VP(h), cx.ptr(rows_in), L, cap, cx.ptr(nrows), None, cx.ptr(seg_in), len(spec["special_ids"]), c_spec, spec["start_prob"], spec["len_lo"],
                                            spec["len_hi"], spec["sentinel_first"], spec["sentinel_step"], spec["max_sentinels"], spec["eos_id"], spec["pad_id"], spec["ignore_label"],
                                            spec["seed"], spec["epoch"], enc_len, o[0], o[1], o[2], dec_len, o[3], o[4], o[5], o[6], cx.stream)
        return r, outs
    step = Step(name, call, want, 0, status, why, size)
    step.denoise = dict(rows=rows, seg=seg, L=L, enc_len=enc_len, dec_len=dec_len, answer=w)
    return step


def denoise_truncated_step(name, size, ids, ido, L=12):
    rows, seg = stream_rows(ids, ido, L)
    return denoise_step(name, size, rows, seg, L, L, DENOISE_TRUNCATED_DEC, 1, "status 1: a row's decoder targets are longer than dec_len (bit 0, set by the kernel's atomic)")


# ---- the secondary calls
def two_pass_step(name, size, fn_name, pre, n, w_flat, w_off, post=(), extras=(), query=False, status=0, why="status 0: the capacity is the exact total", where=None):
    """a Device call of the two-pass kind (IdsToText, DictGetInfo, WordHyphenation): pre = the arguments in front of the output, (array | int), post
    = those behind the offsets; extras = (position in pre, wanted array) of per-item outputs; query: a NULL output, the offsets alone.
    The status is that of the size pass: the fill pass, which runs in the same call, keeps the words the size pass left"""
    total = int(w_off[-1])
    dtype = w_flat.dtype
    want = [] if query else [Want("output", padded(w_flat, total), where or ("docs", w_off))]
    want += [Want("offsets", w_off)] + [Want("per-item result %d" % pos, padded(a, n)) for pos, a in extras]

    def call(h, cx):
        out, o = None if query else cx.full(total + TAIL, dtype), cx.full(n + 1, np.int64)
        ex = [cx.full(n + TAIL, np.int32) for _ in extras]
        args = [cx.ptr(a) if isinstance(a, np.ndarray) else a for a in pre]
        for (pos, _), t in zip(extras, ex):
            args[pos] = t.data_ptr()
        r = getattr(bf.lib(), fn_name)(VP(h), *args, None if query else out.data_ptr(), total, o.data_ptr(), *post, cx.stream)
        return r, ([] if query else [out]) + [o] + ex
    return Step(name, call, want, 0, status, why, size)


# ------------------------------------------------------------------------------------------------
# the catalogues: one per kind of handle
# ------------------------------------------------------------------------------------------------
class Catalogue:
    def __init__(self, kind, path, steps):
        self.kind, self.path, self.steps = kind, path, steps
        assert len({s.name for s in steps}) == len(steps)

    def load(self):
        return bf.load_model(self.path)


def boundary_cap(ido):
    """an ids_cap below the total and above the first document's count, at a document boundary near the middle: every id below it belongs to a document
    that lies wholly inside the buffer, so the whole buffer is determined (nothing at or behind ids_cap is written)"""
    total = int(ido[-1])
    first = int(ido[ido > 0][0])
    cap = int(ido[np.searchsorted(ido, total // 2)])
    assert first < cap < total
    return cap


def tokenizer_matrix(model, pair, variants, sizes=("big", "small")):
    steps = []
    for vname, variant in variants:
        for size in sizes:
            steps.append(tok_device_step("%s %s ids" % (vname, size), size, batch(size), ids_answer(model, size, pair), variant, pair))
            steps.append(tok_device_step("%s %s offsets" % (vname, size), size, batch(size), offsets_answer(model, size, pair), variant, pair))
    return steps


def common_tokenizer_steps(model, pair, flat_variant, overflow_name="big overflow"):
    """the steps every tokenizer catalogue has: an overflow on big (status 1), no document at all, one TextToIds"""
    big = ids_answer(model, "big", pair)
    steps = [tok_device_step(overflow_name, "big", batch("big"), big, flat_variant, pair, cap=boundary_cap(big[3]), status=1,
                             why="status 1: ids_cap is below the id total of the batch (bit 0)"),
             tok_device_step("no documents", "small", empty_batch(), frozen(np.zeros(0, np.int32), None, None, np.zeros(1, np.int64)), 3, pair,
                             why="status 0: ndocs == 0, nothing to report")]
    steps.append(host_single_step("TextToIds", model, small_docs()[7], pair, False))
    return steps


def wordpiece():
    model = bfutil.bert_model_name()
    if not bfutil.have_model(model):
        return None
    pair = WP_PAIR
    steps = tokenizer_matrix(model, pair, (("flat", 4), ("wave", 5), ("lane", 2)))
    steps += common_tokenizer_steps(model, pair, 4, "flat big overflow")
    text, off = small_batch()
    steps.append(tok_device_step("small bad range", "small", (text, bad_range_offsets(off)), ids_answer(model, "small", pair, drop_last=True), 3, pair, status=8,
                                 why="status 8: the last document claims bytes behind total_bytes (bit 3) and is empty; every other document has its answer"))
    small_ids = ids_answer(model, "small", pair)
    steps += [host_batch_step("variant 0 small, mapped", "small", small_ids, 0, pair),
              host_single_step("TextToIdsWithOffsets", model, small_docs()[7], pair, True),
              host_batch_step("TextToIdsBatch small", "small", small_ids, 3, pair),
              host_batch_step("TextToIdsBatch big, chunks of 256 KiB", "big", ids_answer(model, "big", pair), 3, pair, chunk=256 << 10)]
    steps += [words_step("words big", "big", model, 1, 3), words_step("sentences small", "small", model, 2, 3),
              words_step("words small no_long", "small", model, 1, 3 | NO_LONG), words_step("sentences big no_long", "big", model, 2, 3 | NO_LONG)]
    si, ss, se, so = offsets_answer(model, "small", pair)
    bi, bs, be, bo = offsets_answer(model, "big", pair)
    steps += [rows_step("rows L=12 windows small", "small", si, so, 12, 3, 0, narrow=True), rows_step("rows L=64 one row big", "big", bi, bo, 64, 0, 1),
              pair_rows_step("pair rows L=64 QA small", "small", si, so, 64, 8, 4), rows_step("planes L=12 windows big", "big", bi, bo, 12, 2, 0, ((bs, be), (-1, -1))),
              packed_step("packed L=12 big", "big", bi, bo, 12), packed_step("packed L=64 small", "small", si, so, 64),
              span_step("span cells L=64 small", "small", si, so, ss, se, 64), mlm_step("mlm whole words L=12 small", "small", si, so, ss, se, 12)]
    return Catalogue("wordpiece", bfutil.model_path(model), steps)


def unigram():
    model = "xlnet.bin"
    if not bfutil.have_model(model):
        return None
    pair = SP_PAIR
    steps = []
    for vname, variant in (("cut", 3), ("lane", 6), ("quick", 3 | 0x20)):
        for size in ("big", "small"):
            steps.append(tok_device_step("%s %s ids" % (vname, size), size, batch(size), ids_answer(model, size, pair), variant, pair))
    steps += [tok_device_step("big offsets", "big", batch("big"), offsets_answer(model, "big", pair), 3, pair),
              tok_device_step("small offsets", "small", batch("small"), offsets_answer(model, "small", pair), 3, pair)]
    steps += common_tokenizer_steps(model, pair, 3)
    bi, _, _, bo = ids_answer(model, "big", pair)
    si, _, _, so = ids_answer(model, "small", pair)
    steps += [rows_step("rows L=12 windows small", "small", si, so, 12, 3, 0, narrow=True), packed_step("packed L=64 big", "big", bi, bo, 64), mlm_step("mlm L=12 small", "small", si, so, None, None, 12)]
    return Catalogue("unigram", bfutil.model_path(model), steps)


ARC_POOL_DOC = b"-" * 1500                               # tests/test_zz_gpu_bpe_arc_pool.py: more candidate arcs than a document's reserve, far below the default pool


def bpe():
    model = "gpt2.bin"
    if not bfutil.have_model(model):
        return None
    pair = SP_PAIR
    steps = []
    for vname, variant in (("wave", 3), ("lanes", 3 | 0x40)):
        for size in ("big", "small"):
            steps.append(tok_device_step("%s %s ids" % (vname, size), size, batch(size), ids_answer(model, size, pair), variant, pair))
    steps += [tok_device_step("big offsets", "big", batch("big"), offsets_answer(model, "big", pair), 3, pair),
              tok_device_step("small offsets", "small", batch("small"), offsets_answer(model, "small", pair), 3, pair)]

    def pool_batch():
        docs = small_docs()
        docs.insert(20, ARC_POOL_DOC)
        return frozen(*flat_cases.pack(docs))
    ptext, poff = memo("arc pool batch", pool_batch)
    ck, hck = t2i_checker(model)
    pids, pido = memo(("arc pool ids", model), lambda: frozen(*ck.batch(hck, ptext, poff, *pair)))

    def took_the_pool(h):
        f = bf.lib().BfBpeFallbackDocs
        f.restype, f.argtypes = ctypes.c_longlong, [VP]
        return None if f(VP(h)) > 0 else "BfBpeFallbackDocs is %d: no document took the full path" % f(VP(h))
    pool = tok_device_step("small with an arc-pool document", "small", (ptext, poff), (pids, None, None, pido), 3, pair,
                           why="status 0: the document's arcs fit the default pool of 64 MiB (bit 6 stays out)")
    pool.after = took_the_pool
    steps.append(pool)
    steps += common_tokenizer_steps(model, pair, 3)
    import test_dict_lookup
    keys = test_dict_lookup.keys_for(model, n_random=300, seed=3, negative=False)
    dck = sc.DictChecker(model)
    try:
        ret, info, vals, v_off = frozen(*dck.batch(keys))
    finally:
        dck.close()
    k_flat, k_off = frozen(*sc.pack([np.array(k, dtype=np.int32) for k in keys], np.int32))
    n = len(keys)
    assert (np.diff(v_off) > 0).any() and (ret < 0).any()
    dict_pre = [k_flat, k_off, n, None, None]
    dict_why = "status 0: the lookup reports nothing through the status word; it is the call's own since the size pass clears it"
    steps += [two_pass_step("dictionary lookup", "small", "DictGetInfoBatchDevice", dict_pre, n, vals, v_off, extras=[(3, ret), (4, info)], why=dict_why),
              two_pass_step("dictionary lookup, size query", "small", "DictGetInfoBatchDevice", dict_pre, n, vals, v_off, extras=[(3, ret), (4, info)], query=True, why=dict_why)]
    si, _, _, so = ids_answer(model, "small", pair)
    steps.append(rows_step("rows L=12 windows small", "small", si, so, 12, 3, 0, narrow=True))
    return Catalogue("bpe", bfutil.model_path(model), steps)


def i2w_sequences(ntok, n, seed):
    """n id sequences of 0 .. 700 known ids"""
    rnd = np.random.RandomState(seed)
    lens = rnd.choice([0, 1, 2, 5, 20, 64, 65, 100, 700], size=n)
    return [rnd.randint(0, ntok, size=k).astype(np.int32) for k in lens]


def i2w():
    model = "gpt2.i2w"
    if not bfutil.have_model(model):
        return None
    ntok = sc.i2w_count(model)
    ck = memo("secondary checker", sc.Checker)
    hck = memo(("secondary model", model), lambda: ck.load(model))
    seqs = {"big": i2w_sequences(ntok, 1100, 5), "small": i2w_sequences(ntok, 37, 7)}
    unknown = [s.copy() for s in seqs["small"]]
    k = next(i for i, s in enumerate(unknown) if len(s) > 2)
    unknown[k][1] = ntok + 5
    steps, packed_in = [], {}
    for name, size, ss, query, status, why in (("ids to text big", "big", seqs["big"], False, 0, None), ("ids to text small", "small", seqs["small"], False, 0, None),
                                              ("ids to text small, one unknown id", "small", unknown, False, 4,
                                               "status 4: one sequence holds an id outside the model (bit 2) and yields no text"),
                                              ("ids to text big, size query", "big", seqs["big"], True, 0, None)):
        flat, off = frozen(*sc.pack(ss, np.int32))
        packed_in[name] = (flat, off)
        w_flat, w_off = frozen(*sc.pack([ck.ids_to_text(hck, s, 0) for s in ss]))
        if status:
            assert w_off[k + 1] == w_off[k]
        steps.append(two_pass_step(name, size, "IdsToTextBatchDevice", [flat, off, len(ss)], len(ss), w_flat, w_off, post=(0,), query=query, status=status,
                                   why=why or "status 0: every id is known, text_cap is the exact total"))
    one = next(s for s in seqs["small"] if len(s) >= 5)
    text = ck.ids_to_text(hck, one, 0)
    assert text
    w_one = [Want("text", np.concatenate([np.frombuffer(text + b"\0", dtype=np.uint8), np.full(TAIL, 0x7F, dtype=np.uint8)]))]

    def call_one(h, cx):
        out = np.full(len(text) + 1 + TAIL, 0x7F, dtype=np.uint8)
        return bf.lib().IdsToText(VP(h), one.ctypes.data, len(one), out.ctypes.data, len(text) + 1, False), [out]
    steps.append(Step("IdsToText", call_one, w_one, len(text) + 1, 0, "status 0: every id is known"))
    bi, bo = packed_in["ids to text big"]
    si, so = packed_in["ids to text small"]
    steps += [rows_step("rows L=12 windows small", "small", si, so, 12, 3, 0, narrow=True), packed_step("packed L=64 big", "big", bi, bo, 64), mlm_step("mlm L=12 small", "small", si, so, None, None, 12)]
    # a handle without a tokenizer: the stream stage and the denoise call's status 1 meet IdsToText's status 4
    steps += [stream_step("stream L=12 small", "small", si, so, 12, CLS, SEP), denoise_truncated_step("denoise L=12 small, truncated", "small", si, so)]
    return Catalogue("i2w", bfutil.model_path(model), steps)


def w2h():
    import os
    import w2h_cases as wc
    if not os.path.exists(wc.FIXTURE_GZ):
        return None
    en = wc.en_words()
    texts = wc.ref_texts("batch_en", wc.FIXTURE, en)["45"]
    pick = {"big": np.arange(len(en)), "small": (np.arange(37) * 577 + 11) % len(en)}
    steps = []
    for name, size, query, bad in (("hyphenation big", "big", False, False), ("hyphenation small", "small", False, False), ("hyphenation big, size query", "big", True, False),
                                   ("hyphenation small, bad range", "small", False, True)):
        idx = pick[size]
        flat, off = sc.pack([en[i] for i in idx])
        want_texts = [texts[i] for i in idx]
        if bad:
            off = off.copy()
            off[-1] += 1000                              # the last word claims bytes behind the text: it is empty, bit 3
            want_texts[-1] = ""
        w_flat, w_off = wc.pack_texts(want_texts)
        frozen(flat, off, w_flat, w_off)
        steps.append(two_pass_step(name, size, "WordHyphenationBatchDevice", [flat, off, len(idx), len(flat)], len(idx), w_flat.copy(), w_off, post=(0x2D,), query=query,
                                   status=8 if bad else 0, why="status 8: the last word's range leaves the text (bit 3)" if bad else "status 0: every word inside the text"))
    k = next(i for i in pick["small"] if len(texts[i]) > len(en[i]))
    word, text = en[k], texts[k].encode("latin-1")
    cap = 8 * len(word) + 16
    w_one = [Want("text", np.concatenate([np.frombuffer(text + b"\0", dtype=np.uint8), np.full(cap + TAIL - len(text) - 1, 0x7F, dtype=np.uint8)]))]

    def call_one(h, cx):
        out = np.full(cap + TAIL, 0x7F, dtype=np.uint8)
        return bf.lib().WordHyphenationWithModel(word, len(word), out.ctypes.data, cap, VP(h), 0x2D), [out]
    steps.append(Step("WordHyphenationWithModel", call_one, w_one, len(text) + 1, 0, "status 0: one word inside its text"))
    ids, ido = frozen(*packed_cases.mixed(37, 3, 12, CLS, SEP))
    steps.append(rows_step("rows L=12 windows small", "small", ids, ido, 12, 3, 0))
    return Catalogue("w2h", wc.FIXTURE, steps)


STREAM_DROP_WITHIN = stream_cases.DROP_LAST | stream_cases.LABELS_WITHIN


def inputs():
    """the model-input calls on a WordPiece handle: the tokenizer calls that feed them (Device and host), the packed stage with its planes form, the
    stream stage, the capped MLM call beside the base one, span corruption, and a host-buffer form of every row stage.  18 steps, three on the
    big batch; the ids and byte offsets are the checker's, as in wordpiece()"""
    model = bfutil.bert_model_name()
    if not bfutil.have_model(model):
        return None
    pair = WP_PAIR
    si, ss, se, so = offsets_answer(model, "small", pair)
    bi, bs, be, bo = offsets_answer(model, "big", pair)
    steps = [tok_device_step("wave small offsets", "small", batch("small"), (si, ss, se, so), 5, pair),
             tok_device_step("flat big ids", "big", batch("big"), ids_answer(model, "big", pair), 4, pair),
             host_batch_step("TextToIdsBatch small", "small", ids_answer(model, "small", pair), 3, pair),
             packed_step("packed L=12 small", "small", si, so, 12),
             packed_planes_step("packed planes L=12 big", "big", bi, bo, 12, (bs, be), (-1, -1)),
             packed_planes_step("packed planes L=64 small, narrow", "small", si, so, 64, (ss, se, si), (-1, -1, -1), narrow=True, skip_last=True),
             packed_planes_host_step("packed planes host L=12 small", "small", si, so, 12, (ss, se), (-1, -1)),
             rows_planes_host_step("rows planes host L=12 small", "small", si, so, 12, 3, 0, (ss, se), (-1, -1)),
             stream_step("stream L=64 big", "big", bi, bo, 64, CLS, SEP),
             stream_step("stream L=13 small", "small", si, so, 13, -1, SEP, STREAM_DROP_WITHIN)]
    R12 = stream_answer(si, so, 12, CLS, SEP, 0)[8]
    bad = bad_range_offsets(so)
    steps += [stream_step("stream L=12 small overflow", "small", si, so, 12, CLS, SEP, rows_cap=R12 // 2, status=1,
                          why="status 1: rows_cap is below the row count (bit 0); nothing at or past rows_cap is written"),
              stream_step("stream small bad range", "small", si, bad, 12, CLS, SEP, status=8,
                          why="status 8: the last sequence claims ids behind ids_len (bit 3) and is read as empty; every other sequence keeps its answer"),
              stream_step("stream host L=12 small", "small", si, so, 12, CLS, SEP, host=True),
              mlm_step("mlm mask L=64 small", "small", si, so, ss, se, 64),
              predictions_step("mlm predictions L=12 small", "small", si, so, ss, se, 12, PRED_CAP),
              predictions_step("mlm predictions max_pred=0 L=12 small", "small", si, so, ss, se, 12, 0)]
    rows, seg = stream_rows(si, so, 64)
    steps += [denoise_step("denoise L=64 small", "small", rows, seg, 64, 64, 66, 0, "status 0: enc_len = L and dec_len = L + 2 hold every row"),
              denoise_truncated_step("denoise L=12 small, truncated", "small", si, so)]
    return Catalogue("inputs", bfutil.model_path(model), steps)


BUILDERS = {"wordpiece": wordpiece, "unigram": unigram, "bpe": bpe, "i2w": i2w, "w2h": w2h, "inputs": inputs}


def catalogue(kind):
    """the catalogue of a kind of handle, built once; None when its model file is absent"""
    return memo(("catalogue", kind), BUILDERS[kind])


# ------------------------------------------------------------------------------------------------
# comparison
# ------------------------------------------------------------------------------------------------
def describe_difference(want, got):
    """names the first element of a buffer that differs: its document, row or item"""
    got = np.asarray(got).reshape(-1)
    w = want.array.reshape(-1)
    if len(got) != len(w):
        return "%s: %d elements, %d wanted" % (want.label, len(got), len(w))
    at = int(np.flatnonzero(got != w)[0])
    if want.where[0] == "docs":
        off = want.where[1]
        d = int(np.searchsorted(off, at, side="right")) - 1
        place = "behind the last document (the sentinel)" if at >= off[-1] else "document %d, element %d of its %d" % (d, at - off[d], off[d + 1] - off[d])
    elif want.where[0] == "rows":
        place = "row %d, cell %d" % divmod(at - (want.where[2] if len(want.where) > 2 else 0), want.where[1])
    else:
        place = "item %d" % at
    return "%s: %s (element %d of %d): got %s, wanted %s" % (want.label, place, at, len(w), got[at:at + 8].tolist(), w[at:at + 8].tolist())
