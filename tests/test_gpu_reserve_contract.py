"""GPU: the promise of BfReserve (include/blingfiretokdll_amd.h) -- after BfReserve(h, D, B, want_offsets) no ...BatchDevice call on a batch within
(D documents, B bytes) allocates device memory, the FIRST call included -- held to every Device call of the C-ABI, with every program a
BfSetVariant value selects, on batches that touch the bound exactly (tests/reserve_cases.py; tests/test_reserve_cases_host.py proves the inputs).

Every case: load, set the variant (and the BPE pool size), BfReserve, snapshot BfWorkspaceGrows, then for each shape of the bound the Device call on
torch tensors on a side stream; after every call the library's allocation count outside the long-document workspace of the words modes has
not moved, every output equals the CPU checker's (the compiled reference where oracle/_ref is built, else the oracle; the restatements of the
row stages; the stored reference answers of the hyphenation fixture), and BfLastStatus is 0.  The counter sees the library's own hipMalloc
calls alone: torch's allocator and other processes on the card cannot move it, and nothing here reads the card's free memory.

These are also parity checks on workspaces of exactly the reserved size.  A workspace that BfReserve sized too small shows as an allocation, not
as memory corruption: the calls still grow their buffers on demand."""
import ctypes

import numpy as np
import pytest

import bfutil
import blingfire_amd as bf
import denoise_cases
import mlm_cases
import mlmcap_cases
import packed_cases
import packedplanes_cases
import pair_cases
import plane_cases
import reserve_cases as rv
import rows_cases
import secondary_cases as sc
import stream_cases

pytestmark = pytest.mark.gpu

VP = ctypes.c_void_p
NO_LONG = 0x40000000                    # bf_variant.h WordsKnobs::no_long
CLS, SEP, PAD = rows_cases.CLS, rows_cases.SEP, rows_cases.PAD


def torch_():
    import torch
    return torch


class Reserved:
    """a handle with its variant set, reserved for (D, B); check() after a Device call: the allocation counters against the snapshot taken behind BfReserve"""

    def __init__(self, model, D, B, want_offsets=False, variant=None, pool=None, path=None):
        L = bf.lib()
        self.h = bf.load_model(path or bfutil.model_path(model))
        self.what = "%s variant %s reserved (%d, %d, offsets %d)" % (model, "default" if variant is None else hex(variant), D, B, int(want_offsets))
        try:
            if variant is not None:
                assert L.BfSetVariant(VP(self.h), variant) >= 0, self.what
            if pool is not None:
                assert L.BfSetBpePoolBytes(VP(self.h), pool) >= 0, self.what
            bf.reserve(self.h, D, B, want_offsets)
        except BaseException:
            bf.free_model(self.h)
            raise
        self.stream = torch_().cuda.Stream()
        self.base = bf.workspace_grows()
        self.calls = 0

    def check(self, call, long_may_move=False):
        """behind one Device call (the stream is drained first: a grow is counted when it is made, but the status word is read here too)"""
        self.stream.synchronize()
        total, long_ = bf.workspace_grows()
        self.calls += 1
        what = "%s, call %d (%s)" % (self.what, self.calls, call)
        assert total - long_ == self.base[0] - self.base[1], "%s: %d device allocation(s) inside a Device call on a reserved handle" % (
            what, (total - long_) - (self.base[0] - self.base[1]))
        if not long_may_move:
            assert long_ == self.base[1], "%s: the long-document workspace grew %d time(s) in a call that has no use for it" % (what, long_ - self.base[1])
        assert bf.lib().BfLastStatus(VP(self.h)) == 0, what
        return what

    def close(self):
        bf.free_model(self.h)


# ------------------------------------------------------------------------------------------------
# TextToIdsBatchDevice / TextToIdsWithOffsetsBatchDevice
# ------------------------------------------------------------------------------------------------
_expected = {}


def max_ids_of(docs):
    """more ids than any document of the batch can have (a token has at least one stream element, a 1 : n charmap doubles them at most): nothing is cut"""
    return 2 * max([len(d) for d in docs] + [0]) + 16


def expected_ids(model, unk, key, docs):
    """(ids, starts, ends, id_off) of the checker's TextToIdsWithOffsets over `docs`, one document at a time behind a fixed byte (bfutil._T2I.with_offsets,
    with buffers that are allocated once); its TextToIds gives the same ids.  Computed once per (model, bound, shape) and shared by the variants."""
    if (model, key) in _expected:
        return _expected[(model, key)]
    ref = bfutil.have_ref()
    ck = bfutil.reference() if ref else bfutil.oracle()
    f = getattr(ck.lib, "TextToIdsWithOffsets" if ref else "bfo_text_to_ids_with_offsets")
    f.restype = ctypes.c_int
    f.argtypes = [VP, VP, ctypes.c_int, VP, VP, VP, ctypes.c_int, ctypes.c_int]
    mx = max_ids_of(docs)
    bi, bs, be = ((ctypes.c_int32 * mx)() for _ in range(3))
    hck = ck.load(bfutil.model_path(model))
    try:
        ids, st, en, off = [], [], [], np.zeros(len(docs) + 1, dtype=np.int64)
        for d, b in enumerate(docs):
            buf = ctypes.create_string_buffer(b"A" + b, len(b) + 1)
            c = max(f(VP(hck), ctypes.addressof(buf) + 1, len(b), bi, bs, be, mx, unk), 0)
            assert c < mx, (model, key, d)
            for lst, src in ((ids, bi), (st, bs), (en, be)):
                lst.append(np.frombuffer(src, dtype=np.int32, count=c).copy())
            off[d + 1] = off[d] + c
        cat = lambda a: np.concatenate(a) if a else np.zeros(0, dtype=np.int32)
        want = (cat(ids), cat(st), cat(en), off)
        text, doc_off = rv.pack(docs)
        plain, plain_off = ck.batch(hck, text, doc_off, mx, unk)
        assert np.array_equal(plain_off, off) and np.array_equal(plain, want[0]), (model, key, "the checker's two calls disagree")
    finally:
        ck.free(hck)
    _expected[(model, key)] = want
    return want


def run_tokenizer(r, model, unk, D, B, want_offsets, pieces=None, kernel=None):
    torch = torch_()
    L = bf.lib()
    L.BfTokeniseKernel.restype = ctypes.c_char_p
    L.BfTokeniseKernel.argtypes = [VP]
    for name, docs in rv.shapes(D, B, pieces).items():
        want = expected_ids(model, unk, (D, B, name), docs)
        text, off = rv.pack(docs)
        mx = max_ids_of(docs)
        with torch.cuda.stream(r.stream):
            d_text, d_off = torch.from_numpy(text).cuda(), torch.from_numpy(off).cuda()
            ids, id_off = bf.text_to_ids_batch_device(r.h, d_text, d_off, mx, unk, stream=r.stream.cuda_stream)
        what = r.check("TextToIdsBatchDevice, shape %s" % name)
        o = id_off.cpu().numpy()
        assert np.array_equal(o, want[3]), what
        assert np.array_equal(ids[:int(o[-1])].cpu().numpy(), want[0]), what
        if kernel and name in rv.TOUCHING:
            assert L.BfTokeniseKernel(VP(r.h)) in kernel, (what, L.BfTokeniseKernel(VP(r.h)))
        if not want_offsets:
            continue
        with torch.cuda.stream(r.stream):
            got = bf.text_to_ids_with_offsets_batch_device(r.h, d_text, d_off, mx, unk, stream=r.stream.cuda_stream)
        what = r.check("TextToIdsWithOffsetsBatchDevice, shape %s" % name)
        o = got[3].cpu().numpy()
        assert np.array_equal(o, want[3]), what
        for k, part in enumerate(("ids", "starts", "ends")):
            assert np.array_equal(got[k][:int(o[-1])].cpu().numpy(), want[k]), (what, part)


WP = "bert_base_tok.bin"
# (model, unk, variant, bound, charmap pieces, BPE pool bytes, what BfTokeniseKernel answers behind the shapes that touch the bound)
TOKENIZER_CASES = [
    (WP, 100, 4, rv.SMALL, None, None, (b"k_wp_flat",)),
    (WP, 100, 5, rv.SMALL, None, None, (b"k_wp_wave",)),
    (WP, 100, 2, rv.SMALL, None, None, (b"k_lex_wp_plain", b"k_lex_wp_flat")),
    (WP, 100, None, rv.BY_SIZE, None, None, (b"k_wp_flat",)),           # the flat program by the library's own choice
    ("xlnet.bin", 0, 3, rv.SMALL, None, None, (b"k_uni_cut",)),
    ("xlnet.bin", 0, 6, rv.SMALL, None, None, (b"k_seg_unigram_lane",)),
    ("xlm_roberta_base.bin", 3, None, rv.SMALL, "xlmr", None, None),     # the 1 : n charmap, the expanding shape
    ("gpt2.bin", 0, 3, rv.SMALL, None, None, (b"k_bpe_wave",)),
    ("gpt2.bin", 0, 3 | 0x40, rv.SMALL, None, None, (b"k_bpe_fused",)),
    ("gpt2.bin", 0, None, rv.SMALL, None, 128 << 20, None),              # BfSetBpePoolBytes before BfReserve
]


def _case_id(c):
    return "%s-%s-%d%s" % (c[0].split(".")[0], "default" if c[2] is None else hex(c[2]), c[3][0], "-pool" if c[5] else "")


@pytest.mark.parametrize("want_offsets", [0, 1])
@pytest.mark.parametrize("case", TOKENIZER_CASES, ids=_case_id)
def test_text_to_ids_allocates_nothing_after_reserve(case, want_offsets):
    model, unk, variant, (D, B), pieces, pool, kernel = case
    r = Reserved(model, D, B, bool(want_offsets), variant, pool)
    try:
        run_tokenizer(r, model, unk, D, B, bool(want_offsets), pieces, kernel)
    finally:
        r.close()


def test_lane_bpe_with_offsets_allocates_nothing_after_reserve():
    """bpe_example.bin: a plain BPE model, whose offsets call takes the lane BPE kernels with their arc lists and work arrays"""
    D, B = rv.SMALL
    r = Reserved("bpe_example.bin", D, B, True)
    try:
        run_tokenizer(r, "bpe_example.bin", 1, D, B, True)
    finally:
        r.close()


# ------------------------------------------------------------------------------------------------
# the calls with a ragged output of their own: words, sentences, ids to text, dictionary lookups, hyphenation
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def at_scale():
    import test_gpu_secondary_at_scale as m
    return m


@pytest.fixture(scope="module")
def L():
    return bf.lib()


def run_case(r, case, name, long_may_move=False):
    """one Device call of a test_gpu_secondary_at_scale.Case at its full size on the reserved handle's side stream, compared as that module compares:
    offsets, every output element, the canaries behind the output, the per-item results"""
    rc, out, off, extras = case.run_dev(case.T, stream=r.stream)
    assert rc == 0, (r.what, case.what, name, rc)
    what = r.check("%s, shape %s" % (case.what, name), long_may_move)
    case._offsets(off, what)
    case._exact(out, off, case.T, what)
    case._untouched(out, case.T, what)
    for (pos, want), got in zip(case.extras, extras):
        assert np.array_equal(got, want), (what, "per-item result", pos)


@pytest.mark.parametrize("knobs", [NO_LONG | 3, 3], ids=["no_long", "default"])
@pytest.mark.parametrize("model,mode", [("wbd.bin", 1), ("sbd.bin", 2)])
def test_words_and_sentences_allocate_nothing_after_reserve(at_scale, L, model, mode, knobs):
    """with WordsKnobs::no_long neither counter moves; with the default knobs only the long-document workspace may be allocated (BfReserve leaves it
    out, include/blingfiretokdll_amd.h).  The one_long shape is the one whose document k_w2t_copy_long assembles."""
    D, B = rv.SMALL
    ck = sc.Checker()
    hck = ck.load(model)
    r = Reserved(model, D, B, False, knobs)
    try:
        for name, docs in rv.shapes(D, B).items():
            case = at_scale.text_case(L, ck, docs, mode, r.h, hck)
            run_case(r, case, name, long_may_move=not (knobs & NO_LONG))
    finally:
        r.close()
        ck.free(hck)


@pytest.mark.parametrize("model", ["gpt2.i2w", "xlnet.i2w"])
def test_ids_to_text_allocates_nothing_after_reserve(at_scale, L, model):
    D, B = rv.SMALL                                     # D sequences
    ck = sc.Checker()
    hck = ck.load(model)
    ntok = sc.i2w_count(model)
    r = Reserved(model, D, B)
    try:
        for name, lens in rv.seq_shapes(D).items():
            rnd = np.random.RandomState(len(lens) + 7)
            seqs = [rnd.randint(0, ntok, size=n).astype(np.int32) for n in lens]
            for skip in (0, 1):
                run_case(r, at_scale.i2t_case(L, r.h, ck, hck, seqs, skip, what="IdsToText " + model), name)
    finally:
        r.close()
        ck.free(hck)


@pytest.mark.parametrize("model", ["gpt2.bin", "xlm_roberta_base.bin"])
def test_dict_get_info_allocates_nothing_after_reserve(at_scale, L, model):
    """the tables of the [pos-dict] go up in BfReserve, not in the first lookup"""
    import test_dict_lookup
    D, B = rv.SMALL                                     # D keys
    pool = test_dict_lookup.keys_for(model, n_random=200, seed=5, negative=False)
    pool = [k for k in pool if 0 < len(k) < 40]
    long_key = [0x2581] + [97] * 300
    dck = sc.DictChecker(model)
    r = Reserved(model, D, B)
    try:
        step = len(pool) // D
        shapes = {"even": pool[::step][:D], "one_long": [long_key if i == D // 2 else [] for i in range(D)], "ones": [[97 + i % 26] for i in range(D)],
                  "empty": [], "half": pool[1::step][:D // 2]}
        assert len(shapes["even"]) == D
        hits = 0
        for name, keys in shapes.items():
            case = at_scale.dict_case(L, r.h, dck, keys, model=model)
            hits += int((np.diff(case.want_off) > 0).sum())
            run_case(r, case, name)
        assert hits > D // 4, (model, hits)
    finally:
        r.close()
        dck.close()


def test_word_hyphenation_allocates_nothing_after_reserve(at_scale, L):
    import test_w2h
    import w2h_cases as wc
    D, B = rv.SMALL                                     # D words
    want = rv.hyphenation_expected()
    r = Reserved("syllab.bin", D, B, path=wc.FIXTURE)
    try:
        for name, words in rv.hyphenation_words().items():
            run_case(r, test_w2h.w2h_case(L, r.h, words, want[name], 0x2D, what="reserve"), name)
        assert sum(len(t) for t in want["even"]) > sum(len(w) for w in rv.hyphenation_words()["even"])      # hyphens were put in
    finally:
        r.close()


# ------------------------------------------------------------------------------------------------
# the row stages: on a WordPiece handle and on an [i2w]-only handle (every kind of handle has their workspaces).  The planes form of the packed
# call and the stream rows live in the packed stage's workspaces; the MLM, predictions and denoise calls have none, and run here over the rows
# the packed and the rows call of the same handle just left on the device
# ------------------------------------------------------------------------------------------------
ROW_L, ROW_STRIDE = 16, 4


def _dev(stream, *arrays):
    torch = torch_()
    with torch.cuda.stream(stream):
        return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


def _same(got, want, what):
    for k, (g, w) in enumerate(zip(got, want)):
        g = g.cpu().numpy()
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), (what, "output", k)


def _two_sides(lens):
    a = pair_cases.ragged(lens, pair_cases.A0)
    b = pair_cases.ragged(lens[::-1], pair_cases.B0)
    return a, b


def stage_rows(r, lens, name):
    ids, off = packed_cases.ragged(lens)
    d_ids, d_off = _dev(r.stream, ids, off)
    with torch_().cuda.stream(r.stream):
        got = bf.ids_to_rows_batch_device(r.h, d_ids, d_off, ROW_L, CLS, SEP, PAD, ROW_STRIDE, 0, False, stream=r.stream.cuda_stream)
    what = r.check("IdsToRowsBatchDevice, shape %s" % name)
    want = rows_cases.restate(ids, off, ROW_L, CLS, SEP, PAD, ROW_STRIDE, 0, False)
    _same(got, want[:5], what)
    return got, want


def stage_pairs(r, lens, name):
    (ia, oa), (ib, ob) = _two_sides(lens)
    da, doa, db, dob = _dev(r.stream, ia, oa, ib, ob)
    with torch_().cuda.stream(r.stream):
        got = bf.ids_to_pair_rows_batch_device(r.h, da, doa, db, dob, ROW_L, CLS, SEP, PAD, 1, stream=r.stream.cuda_stream)
    what = r.check("IdsToPairRowsBatchDevice, shape %s" % name)
    _same(got, pair_cases.restate(ia, oa, ib, ob, ROW_L, CLS, SEP, PAD, 1, 0, 0, 1)[:6], what)


def _token_spans(n):
    """first and last byte of n tokens of three bytes each, as the offsets call would give them"""
    st = (3 * np.arange(n)).astype(np.int32)
    return st, st + 2


def stage_rows_planes(r, lens, name):
    ids, off = packed_cases.ragged(lens)
    src = list(_token_spans(len(ids)))
    d_ids, d_off, s0, s1 = _dev(r.stream, ids, off, *src)
    with torch_().cuda.stream(r.stream):
        *base, planes = bf.ids_to_rows_planes_batch_device(r.h, d_ids, d_off, ROW_L, CLS, SEP, PAD, ROW_STRIDE, 0, False, stream=r.stream.cuda_stream,
                                                           src=[s0, s1], fill=[-1, -1])
    what = r.check("IdsToRowsPlanesBatchDevice, shape %s" % name)
    w_planes, w_seq, w_first, w_off, _ = plane_cases.restate_planes(off, ROW_L, CLS, SEP, ROW_STRIDE, 0, False, src, [-1, -1])
    _same(planes, w_planes, what)
    _same(base[2:], (w_seq, w_first, w_off), what)
    return planes, base[2], base[4], w_planes, w_seq


def stage_pair_planes(r, lens, name):
    (ia, oa), (ib, ob) = _two_sides(lens)
    src_a, src_b = plane_cases.sources(len(ia), 2, 5, plane_cases.FILLS), plane_cases.sources(len(ib), 2, 6, plane_cases.FILLS)
    da, doa, db, dob, a0, a1, b0, b1 = _dev(r.stream, ia, oa, ib, ob, *src_a, *src_b)
    with torch_().cuda.stream(r.stream):
        *base, planes = bf.ids_to_pair_rows_planes_batch_device(r.h, da, doa, db, dob, ROW_L, CLS, SEP, PAD, 1, stream=r.stream.cuda_stream,
                                                                src_a=[a0, a1], src_b=[b0, b1], fill=plane_cases.FILLS[:2])
    what = r.check("IdsToPairRowsPlanesBatchDevice, shape %s" % name)
    w_planes, w_seq, w_first, w_off, _ = plane_cases.restate_pair_planes(oa, ob, ROW_L, CLS, SEP, 1, 0, 0, 1, False, False, src_a, src_b, plane_cases.FILLS[:2])
    _same(planes, w_planes, what)
    _same(base[3:], (w_seq, w_first, w_off), what)


def stage_span_cells(r, lens, name):
    planes, d_seq, d_roff, w_planes, w_seq = stage_rows_planes(r, lens, name)
    nseq = len(lens)
    first = np.array([3 * (n // 3) for n in lens], dtype=np.int32)                         # a byte inside the sequence's tokens (none for an empty one)
    last = np.array([3 * (n // 3) + 4 if n else -1 for n in lens], dtype=np.int32)
    d_first, d_last = _dev(r.stream, first, last)
    with torch_().cuda.stream(r.stream):
        got = bf.rows_span_cells_device(r.h, planes[0], planes[1], d_seq, d_roff, d_first, d_last, 0, stream=r.stream.cuda_stream)
    what = r.check("RowsSpanCellsBatchDevice, shape %s" % name)
    _same(got, plane_cases.restate_span_array(w_planes[0], w_planes[1], w_seq, nseq, first, last, 0)[:2], what)


def stage_packed(r, lens, name):
    ids, off = packed_cases.ragged(lens)
    d_ids, d_off = _dev(r.stream, ids, off)
    with torch_().cuda.stream(r.stream):
        got = bf.ids_to_packed_rows_batch_device(r.h, d_ids, d_off, ROW_L, CLS, SEP, PAD, stream=r.stream.cuda_stream)
    what = r.check("IdsToPackedRowsBatchDevice, shape %s" % name)
    want = packed_cases.restate(ids, off, ROW_L, CLS, SEP, PAD)
    _same(got[:6], want[:6], what)
    assert int(got[6].item()) == want[6], what
    return got, want


def stage_packed_planes(r, lens, name):
    """the planes form of the packed call: one kernel behind the base call's, over what that call left in the packed stage's workspaces"""
    ids, off = packed_cases.ragged(lens)
    src = list(_token_spans(len(ids)))
    d_ids, d_off, s0, s1 = _dev(r.stream, ids, off, *src)
    with torch_().cuda.stream(r.stream):
        got = bf.ids_to_packed_rows_batch_device(r.h, d_ids, d_off, ROW_L, CLS, SEP, PAD, stream=r.stream.cuda_stream, planes=[s0, s1], fill=[-1, -1])
    what = r.check("IdsToPackedRowsPlanesBatchDevice, shape %s" % name)
    want = packed_cases.restate(ids, off, ROW_L, CLS, SEP, PAD)
    _same(got[:6], want[:6], what)
    assert int(got[6].item()) == want[6] and len(got) == 9, what
    _same(got[7:], packedplanes_cases.restate_packed_planes(off, ROW_L, CLS, SEP, src, [-1, -1], ids_len=len(ids)), what)


def stage_stream(r, lens, name):
    """stream rows with both specials, at every row length of rv.STREAM_ROW_LENS: on `one_long` the rows are several times the sequences (R is not bounded
    by nseq), and the claim that no workspace is sized by the row count is on trial (tests/test_reserve_cases_host.py counts the rows)"""
    ids, off = packed_cases.ragged(lens)
    d_ids, d_off = _dev(r.stream, ids, off)
    for L in rv.STREAM_ROW_LENS:
        with torch_().cuda.stream(r.stream):
            got = bf.ids_to_stream_rows_batch_device(r.h, d_ids, d_off, L, CLS, SEP, PAD, stream=r.stream.cuda_stream)
        what = r.check("IdsToStreamRowsBatchDevice, row_len %d, shape %s" % (L, name))
        want = stream_cases.restate_np(ids, off, L, CLS, SEP, PAD)
        assert want[8] == rv.stream_row_count(lens, L) and want[10] == 0, what
        _same(got[:8], want[:8], what)
        assert got[8].tolist() == [want[8], want[9]], what


MLM_SPECIALS = (CLS, SEP, PAD)
MLM_KW = dict(special_ids=MLM_SPECIALS, probs=mlmcap_cases.PROBS, mask_id=mlm_cases.MASK, rand_range=mlm_cases.RAND_RANGE, ignore_label=-100, seed=0x51ED, epoch=2)
MLM_MAX_PRED = 2
DENOISE_KW = dict(denoise_cases.DEFAULTS, special_ids=MLM_SPECIALS, eos_id=SEP, pad_id=PAD, seed=0x51ED, epoch=2)


def _row_sources(r, lens, name):
    """the rows of stage_packed (with their segment plane) and of stage_rows (with their mask) of this call sequence, as the calls left them on the
    device, each with its row bound and with the restated rows: (rows, keywords of the planes and the bound, restated rows, mask, seg)"""
    pg, pw = stage_packed(r, lens, name)
    rg, rw = stage_rows(r, lens, name)
    return [("packed rows", pg[0], dict(seg=pg[1], nrows=pg[6]), (pw[0], None, pw[1])), ("rows", rg[0], dict(mask=rg[1], nrows=rg[4][-1:]), (rw[0], rw[1], None))]


def stage_mlm(r, lens, name, max_pred=0):
    """RowsMlmMaskBatchDevice (max_pred 0) / RowsMlmPredictionsBatchDevice: no workspace, so the counter must not move"""
    for src, d_rows, planes, (w_rows, w_mask, w_seg) in _row_sources(r, lens, name):
        with torch_().cuda.stream(r.stream):
            got = bf.rows_mlm_mask_device(r.h, d_rows, **planes, special_ids=MLM_SPECIALS, select_prob=MLM_KW["probs"][0], mask_prob=MLM_KW["probs"][1], random_prob=MLM_KW["probs"][2],
                                          mask_id=MLM_KW["mask_id"], rand_range=MLM_KW["rand_range"], seed=MLM_KW["seed"], epoch=MLM_KW["epoch"], stream=r.stream.cuda_stream,
                                          max_predictions=max_pred)
        what = r.check("%s over %s, shape %s" % ("RowsMlmPredictionsBatchDevice" if max_pred else "RowsMlmMaskBatchDevice", src, name))
        if max_pred:
            want = mlmcap_cases.restate_cap(w_rows, w_mask, w_seg, max_pred=max_pred, **MLM_KW)
        else:
            want = mlm_cases.restate_mlm(w_rows, w_mask, w_seg, **MLM_KW)
        assert len(got) == len(want), what
        _same(got, want, what)


def stage_denoise(r, lens, name):
    """RowsDenoiseBatchDevice with enc_len = L and dec_len = L + 2, which lose no cell (status 0): no workspace either"""
    names = dict(input_ids="enc", labels="dec", enc_count="enc_count", dec_count="dec_count", span_count="span_count", enc_cells="enc_cell", dec_cells="dec_cell")
    kw = {k: v for k, v in DENOISE_KW.items()}
    for src, d_rows, planes, (w_rows, w_mask, w_seg) in _row_sources(r, lens, name):
        with torch_().cuda.stream(r.stream):
            got = bf.rows_denoise_device(r.h, d_rows, **planes, return_cells=True, stream=r.stream.cuda_stream, **kw)
        what = r.check("RowsDenoiseBatchDevice over %s, shape %s" % (src, name))
        want = denoise_cases.restate_denoise(w_rows, w_mask, w_seg, **kw)
        assert want["status"] == 0 and set(got) == set(names), what
        _same([got[k] for k in names], [want[n] for n in names.values()], what)


STAGES = {"rows": stage_rows, "pair_rows": stage_pairs, "rows_planes": stage_rows_planes, "pair_rows_planes": stage_pair_planes, "span_cells": stage_span_cells,
          "packed_rows": stage_packed, "packed_rows_planes": stage_packed_planes, "stream_rows": stage_stream, "mlm_mask": stage_mlm,
          "mlm_predictions": lambda r, lens, name: stage_mlm(r, lens, name, MLM_MAX_PRED), "denoise": stage_denoise}


@pytest.mark.parametrize("stage", list(STAGES))
@pytest.mark.parametrize("model", [WP, "gpt2.i2w"])
def test_row_stages_allocate_nothing_after_reserve(model, stage):
    D, B = rv.SMALL                                     # D sequences or pairs
    r = Reserved(model, D, B)
    try:
        for name, lens in rv.seq_shapes(D, long_len=300).items():
            STAGES[stage](r, lens, name)
    finally:
        r.close()


# ------------------------------------------------------------------------------------------------
# text to model inputs: the tokenizer and the stages behind it in one wrapper call, on the WordPiece handle
# ------------------------------------------------------------------------------------------------
UNK = 100
SENTINEL_FIRST = 30521                  # made-up sentinel ids: the last ids of the BERT vocabulary, downwards


def test_text_to_model_inputs_allocates_nothing_after_reserve():
    """encode_clm_batch_device, encode_denoise_batch_device (both sources) and encode_packed_mlm_batch_device on a handle reserved with
    want_offsets, on the text shapes that touch the bound with many documents (`even`) and with one long one (`one_long`: the stream rows are
    several times the documents).  Every output is the restatement's over the tokenizer checker's ids and byte offsets."""
    torch = torch_()
    D, B = rv.SMALL
    L = ROW_L
    names = dict(input_ids="enc", labels="dec", enc_count="enc_count", dec_count="dec_count", span_count="span_count", enc_cells="enc_cell", dec_cells="dec_cell")
    dn = dict(start_prob=0.2, len_lo=1, len_hi=4, sentinel_first=SENTINEL_FIRST, sentinel_step=-1, max_sentinels=100, seed=31, epoch=2)
    r = Reserved(WP, D, B, True)
    try:
        shapes = rv.shapes(D, B)
        for name in ("even", "one_long"):
            docs = shapes[name]
            ids, st, en, off = expected_ids(WP, UNK, (D, B, name), docs)
            text, doc_off = rv.pack(docs)
            d_text, d_off = _dev(r.stream, text, doc_off)

            # causal LM: every id of every document, [CLS] and [SEP] around it
            with torch.cuda.stream(r.stream):
                got = bf.encode_clm_batch_device(r.h, d_text, d_off, L, CLS, SEP, PAD, UNK)
            what = r.check("encode_clm_batch_device, shape %s" % name)
            want = stream_cases.restate_np(ids, off, L, CLS, SEP, PAD)
            R, T = want[8], want[9]
            assert got["nrows"].tolist() == [R, T] and got["input_ids"].shape[0] >= R, what
            if name == "one_long":
                assert R > 3 * D, (what, R)
            _same([got[k][:R] for k in list(got)[:6]] + [got["seq_row"], got["seq_col"]], want[:8], what)

            # span corruption over stream rows (no bos, [SEP] closes a document) ...
            with torch.cuda.stream(r.stream):
                got = bf.encode_denoise_batch_device(r.h, d_text, d_off, L, SEP, PAD, SENTINEL_FIRST, dn["seed"], epoch=dn["epoch"], source="stream", unk=UNK,
                                                     start_prob=dn["start_prob"], len_hi=dn["len_hi"], return_cells=True)
            what = r.check("encode_denoise_batch_device from stream rows, shape %s" % name)
            rows = stream_cases.restate_np(ids, off, L, -1, SEP, PAD)
            n = rows[8]
            assert int(got["nrows"].item()) == n > 0, what
            _same([got["rows"][:n], got["seg"][:n]], rows[:2], what)
            want = denoise_cases.restate_denoise(rows[0], None, rows[1], special_ids=sorted({SEP, PAD}), eos_id=SEP, pad_id=PAD, **dn)
            assert want["status"] == 0 and (want["span_count"] > 0).any(), what
            _same([got[k][:n] for k in names], [want[v] for v in names.values()], what)

            # ... and over one truncated row per document
            with torch.cuda.stream(r.stream):
                got = bf.encode_denoise_batch_device(r.h, d_text, d_off, L, SEP, PAD, SENTINEL_FIRST, dn["seed"], epoch=dn["epoch"], source="rows", unk=UNK,
                                                     start_prob=dn["start_prob"], len_hi=dn["len_hi"], return_cells=True)
            what = r.check("encode_denoise_batch_device from rows, shape %s" % name)
            w_rows, w_mask = rows_cases.restate(ids, off, L, -1, SEP, PAD, 0, 1, False)[:2]
            assert int(got["nrows"].item()) == D == len(w_rows), what
            _same([got["rows"], got["mask"]], [w_rows, w_mask], what)
            want = denoise_cases.restate_denoise(w_rows, w_mask, None, special_ids=sorted({SEP, PAD}), eos_id=SEP, pad_id=PAD, **dn)
            assert want["status"] == 0, what
            _same([got[k] for k in names], [want[v] for v in names.values()], what)

            # whole-word MLM over packed rows: the offsets call, the packed call with its planes, the MLM call
            with torch.cuda.stream(r.stream):
                got = bf.encode_packed_mlm_batch_device(r.h, d_text, d_off, L, CLS, SEP, PAD, mlm_cases.MASK, mlm_cases.RAND_RANGE, seed=MLM_KW["seed"], epoch=MLM_KW["epoch"],
                                                        unk=UNK, select_prob=MLM_KW["probs"][0])
            what = r.check("encode_packed_mlm_batch_device, shape %s" % name)
            pk = packed_cases.restate(ids, off, L, CLS, SEP, PAD)
            S, E = packedplanes_cases.restate_packed_planes(off, L, CLS, SEP, [st, en], [-1, -1], ids_len=len(ids))
            w_ids, w_labels = mlm_cases.restate_mlm(pk[0], None, pk[1], S, E, special_ids=MLM_SPECIALS, probs=(MLM_KW["probs"][0],) + mlm_cases.DEFAULT_PROBS[1:],
                                                    seed=MLM_KW["seed"], epoch=MLM_KW["epoch"])
            assert len(got) == 10 and int(got[6].item()) == pk[6], what
            _same(got[:6] + got[7:], [w_ids] + list(pk[1:6]) + [S, E, w_labels], what)
            assert (w_labels != -100).any(), what
    finally:
        r.close()
