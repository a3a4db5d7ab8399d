"""GPU: the ...BatchDevice calls of the C-ABI on the pointers a caller may pass -- include/blingfiretokdll_amd.h asks for the natural alignment of
the element type and nothing else, says that d_text needs no padding and may be d_text + first_byte of a larger buffer, and that no output is written
at or past its capacity.  Every other GPU test passes the base of a fresh torch tensor for every pointer, so the code the kernels keep for these
callers never ran there: k_prep_wp in place of k_prep_wp_flat + k_prep_wp_docs for a text that is not 16-byte aligned (launch_prep_wp), the head /
oq / rows_ok logic of k_wp_merge and its element-wise path for starts_out / ends_out that are not aligned like ids_out, the wide stores k_rowstage_fill
chooses from the alignment of rows / mask, and the end-of-text special cases (wf_units' b16, k_prep_wp_flat's last chunk, the nb < 8 tails of
load_chunk and k_prep_sp8) that keep a kernel from looking at what lies behind total_bytes.

Here every input lies INSIDE a larger device tensor (pointer_cases.place: 4 KiB and more of chosen bytes in front of and behind it, the payload at
a chosen byte shift) and every output inside a canary-filled one (pointer_cases.room).  What surrounds the text is chosen to change the answer if it
is taken in: a lead byte in front and its continuation byte, the rest of a word, a U+2581 and a special token behind ("completing"), 0xFF on both
sides, zeros.  Every expectation is the CPU checker's (the compiled reference where oracle/_ref is built, else the oracle; secondary_cases.Checker
for the secondary calls; the stored reference answers of tests/test_w2h.py for the hyphenator; rows_cases' restatement for the rows) for the PAYLOAD
ALONE; every comparison is exact and covers every document; after every call the canaries in front of and behind each output and every byte of
each input arena are checked.  Nothing here can fault a device that runs a correct or an off-by-a-few-bytes kernel: every address such a kernel
touches is inside a tensor of the test's own."""
import ctypes

import numpy as np
import pytest

import bfutil
import flat_cases
import pointer_cases as pc
import rows_cases as rc
import secondary_cases as sc

pytestmark = pytest.mark.gpu

VP = ctypes.c_void_p
OFFSETS_NAME = "TextToIdsWithOffsets" if bfutil.have_ref() else "bfo_text_to_ids_with_offsets"
SUR = pc.SURROUNDINGS
SUR_NAMES = tuple(SUR)
# model -> (max_ids, unk, variants of section a, variants of section b, variants of section c)
TOKENIZERS = {
    "bert_base_tok.bin": (512, 100, (4, 5, 2, 3), (4, 5), (4, 5, 2)),
    "xlm_roberta_base.bin": (1024, 3, (3, 6), (3,), (3,)),
    "gpt2.bin": (2048, 0, (3, 3 | 0x40), (3,), (3,)),
}


def _params(which):
    return [(m, v) for m, t in TOKENIZERS.items() for v in t[2 + which]]


def _id(p):
    return "%s-v%d" % (p[0].split(".")[0], p[1]) if isinstance(p, tuple) else str(p)


def sync_stream():
    import torch
    torch.cuda.current_stream().synchronize()


def cur_stream():
    import torch
    return VP(torch.cuda.current_stream().cuda_stream)


# ------------------------------------------------------------------------------------------------
# the CPU checker's answers, per distinct document, asked once
# ------------------------------------------------------------------------------------------------
class Tokenizer:
    """a product handle and the checker's handle of one model; want_ids / want_offsets: the checker's TextToIds / TextToIdsWithOffsets of every
    document of a list, concatenated, with the id offsets"""

    def __init__(self, model):
        import blingfire_amd as bf
        self.model = model
        self.max_ids, self.unk = TOKENIZERS[model][:2]
        self.ck = bfutil.reference() if bfutil.have_ref() else bfutil.oracle()
        self.hck = self.ck.load(bfutil.model_path(model))
        self.h = bf.load_model(bfutil.model_path(model))
        self.L = bf.lib()
        self._ids, self._offs = {}, {}
        self._buf = (ctypes.c_int32 * self.max_ids)()

    def close(self):
        import blingfire_amd as bf
        bf.free_model(self.h)
        self.ck.free(self.hck)

    def variant(self, v):
        self.L.BfSetVariant(VP(self.h), v)

    def status(self):
        return self.L.BfLastStatus(VP(self.h))

    def ids_of(self, b):
        if b not in self._ids:
            c = self.ck._t2i(VP(self.hck), b, len(b), self._buf, self.max_ids, self.unk)
            self._ids[b] = np.frombuffer(self._buf, dtype=np.int32, count=min(max(c, 0), self.max_ids)).copy()
        return self._ids[b]

    def offsets_of(self, b):
        if b not in self._offs:
            c, i, s, e = self.ck.with_offsets(self.hck, b, min(self.max_ids, 4 * len(b) + 8), self.unk, OFFSETS_NAME)
            c = min(len(i), self.max_ids)
            self._offs[b] = tuple(np.asarray(x[:c], dtype=np.int32) for x in (i, s, e))
        return self._offs[b]

    @staticmethod
    def _cat(per_doc, k):
        off = np.zeros(len(per_doc) + 1, dtype=np.int64)
        np.cumsum([len(x[k]) for x in per_doc], out=off[1:])
        return off

    def want_ids(self, docs):
        per = [(self.ids_of(b),) for b in docs]
        return np.concatenate([x[0] for x in per] + [np.zeros(0, dtype=np.int32)]), self._cat(per, 0)

    def want_offsets(self, docs):
        per = [self.offsets_of(b) for b in docs]
        z = [np.zeros(0, dtype=np.int32)]
        return tuple(np.concatenate([x[k] for x in per] + z) for k in range(3)) + (self._cat(per, 0),)


_tok = {}


@pytest.fixture(scope="module")
def tokenizer():
    def get(model):
        if model not in _tok:
            _tok[model] = Tokenizer(model)
        return _tok[model]
    yield get
    for t in _tok.values():
        t.close()
    _tok.clear()


_batches = {}


def big_batch(model):
    """section a / b: the WordPiece mixture (streamed, handed-back, invalid and empty documents, about 1.2 MB); 1,500 adversarial and fuzz documents
    for the SentencePiece models.  -> (docs, text, offsets), built once, never changed"""
    kind = "wp" if model.startswith("bert") else "sp"
    if kind not in _batches:
        docs = flat_cases.docs_of(flat_cases.mixture()) if kind == "wp" else (list(bfutil.ADVERSARIAL) + bfutil.fuzz_docs(1500 - len(bfutil.ADVERSARIAL), seed=77))
        text, off = flat_cases.pack(docs)
        text.flags.writeable = False; off.flags.writeable = False
        _batches[kind] = (docs, text, off)
    return _batches[kind]


def first_bad_doc(docs, got_off, want_off, pairs):
    """message naming the first document whose output differs"""
    for d in range(len(docs)):
        if got_off[d + 1] - got_off[d] != want_off[d + 1] - want_off[d]:
            return "document %d of %d %r: %d ids, the checker %d" % (d, len(docs), docs[d][:60], got_off[d + 1] - got_off[d], want_off[d + 1] - want_off[d])
        for what, g, w in pairs:
            a, b = g[want_off[d]:want_off[d + 1]], w[want_off[d]:want_off[d + 1]]
            if not np.array_equal(a, b):
                return "document %d of %d (%d bytes) %r: %s gpu %s != checker %s" % (d, len(docs), len(docs[d]), docs[d][-60:], what, a[:40].tolist(), b[:40].tolist())
    return "the id offsets differ behind the last document"


def run_ids(t, docs, text, off, want, tshift, sur, doff_shift=0, ids_shift=0, idoff_shift=0, ctx=""):
    """TextToIdsBatchDevice with ids_cap = the exact total: ids, offsets, status 0, canaries, input arenas"""
    wids, woff = want
    nd, total = len(off) - 1, int(woff[-1])
    front, back = SUR[sur]
    ptext = pc.place(text, tshift, front, back)
    poff = pc.place(off, doff_shift, b"\xff", b"\xff")
    ids = pc.room(np.int32, total, ids_shift)
    ido = pc.room(np.int64, nd + 1, idoff_shift // 8)
    r = t.L.TextToIdsBatchDevice(VP(t.h), ptext.addr, poff.addr, nd, len(text), ids.addr, total, ido.addr, t.max_ids, t.unk, cur_stream())
    sync_stream()
    what = "%s TextToIdsBatchDevice %s text +%d in '%s', doc offsets +%d, ids +%d items, id offsets +%d" % (t.model, ctx, tshift, sur, doff_shift, ids_shift, idoff_shift)
    assert r == 0, what
    st = t.status()
    g_off, g_ids = ido.fetch().result(), ids.fetch().result()
    if not (np.array_equal(g_off, woff) and np.array_equal(g_ids, wids)):
        raise AssertionError(what + ": " + first_bad_doc(docs, g_off, woff, [("ids", g_ids, wids)]))
    assert st == 0, (what, st)
    ids.untouched(total, what + ", ids")
    ido.untouched(nd + 1, what + ", id offsets")
    ptext.verify(what + ", text")
    poff.verify(what + ", doc offsets")


def run_offsets(t, docs, text, off, want, tshift, sur, shifts=(0, 0, 0), short=0, doff_shift=0, idoff_shift=0, ctx=""):
    """TextToIdsWithOffsetsBatchDevice with cap = the exact total - short.  short > 0: status bit 0, complete offsets, the documents that end at or before
    cap exact, nothing at or behind cap"""
    wids, ws, we, woff = want
    nd, total = len(off) - 1, int(woff[-1])
    cap = total - short
    assert cap > 0
    front, back = SUR[sur]
    ptext = pc.place(text, tshift, front, back)
    poff = pc.place(off, doff_shift, b"\xff", b"\xff")
    outs = [pc.room(np.int32, total, s) for s in shifts]
    ido = pc.room(np.int64, nd + 1, idoff_shift // 8)
    r = t.L.TextToIdsWithOffsetsBatchDevice(VP(t.h), ptext.addr, poff.addr, nd, len(text), outs[0].addr, outs[1].addr, outs[2].addr, cap, ido.addr, t.max_ids, t.unk,
                                            cur_stream())
    sync_stream()
    what = "%s TextToIdsWithOffsetsBatchDevice %s text +%d in '%s', outputs +%s items, cap %d of %d" % (t.model, ctx, tshift, sur, list(shifts), cap, total)
    assert r == 0, what
    st = t.status()
    g_off = ido.fetch().result()
    got = [o.fetch().result() for o in outs]
    done = total if not short else int(woff[np.searchsorted(woff, cap, side="right") - 1])          # the end of the last document that ends at or before cap
    if not (np.array_equal(g_off, woff) and all(np.array_equal(g[:done], w[:done]) for g, w in zip(got, (wids, ws, we)))):
        nfit = int(np.searchsorted(woff, done, side="right")) - 1 if short else nd
        raise AssertionError(what + ": " + first_bad_doc(docs[:nfit] if np.array_equal(g_off, woff) else docs, g_off, woff,
                                                         [("ids", got[0], wids), ("first bytes", got[1], ws), ("last bytes", got[2], we)]))
    assert st == (1 if short else 0), (what, st)
    for o, name in zip(outs, ("ids", "first bytes", "last bytes")):
        o.untouched(cap, what + ", " + name)
    ido.untouched(nd + 1, what + ", id offsets")
    ptext.verify(what + ", text")
    poff.verify(what + ", doc offsets")


# ------------------------------------------------------------------------------------------------
# a. TextToIdsBatchDevice at every text alignment
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mv", _params(0), ids=_id)
def test_a_text_to_ids_at_every_text_alignment(tokenizer, mv):
    """every shift of TEXT_SHIFTS; d_doc_offsets and d_id_offsets_out at 0 and 8 bytes, d_ids_out at 0..3 items behind a 16-byte boundary and the three
    surroundings rotate over them (every value is met four times and more).

    launch_prep_wp takes k_prep_wp for a text that is not 16-byte aligned and k_prep_wp_flat + k_prep_wp_docs otherwise (the lane variant, 2).
    BfStepKernels does not tell the two apart: its string depends on the model kind and the variant, not on the pointers of the last call
    (bf_capi.cpp), so the routing is not asserted here; what is asserted is that both roads give the checker's ids at every shift."""
    model, variant = mv
    t = tokenizer(model)
    docs, text, off = big_batch(model)
    want = t.want_ids(docs)
    t.variant(variant)
    try:
        seen = {}
        for i, shift in enumerate(pc.TEXT_SHIFTS):
            doff, idsh, idoff, sur = 8 * ((i // 2 + i) % 2), (i // 2) % 4, 8 * ((i // 3) % 2), SUR_NAMES[i % 3]
            run_ids(t, docs, text, off, want, shift, sur, doff, idsh, idoff, ctx="variant %d" % variant)
            for k in (("doff", doff), ("ids", idsh), ("idoff", idoff), ("sur", sur)):
                seen[k] = seen.get(k, 0) + 1
        assert len(seen) == 2 + 4 + 2 + 3 and min(seen.values()) >= 4, seen
    finally:
        t.variant(3)


# ------------------------------------------------------------------------------------------------
# b. TextToIdsWithOffsetsBatchDevice with the three outputs aligned differently
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("short", [0, 3], ids=["cap_exact", "cap_minus_3"])
@pytest.mark.parametrize("mv", _params(1), ids=_id)
def test_b_offsets_outputs_aligned_differently(tokenizer, mv, short):
    """every entry of OUT_SHIFTS_3 (12 of the 16 with starts_out / ends_out not aligned like ids_out: k_wp_merge's element-wise path) at text shifts 0
    and 5, with cap = the exact total and with cap = total - 3 (status bit 0, complete offsets, the documents in front of cap exact)"""
    model, variant = mv
    t = tokenizer(model)
    docs, text, off = big_batch(model)
    want = t.want_offsets(docs)
    assert np.array_equal(want[3], t.want_ids(docs)[1]) and np.array_equal(want[0], t.want_ids(docs)[0])
    t.variant(variant)
    try:
        for i, shifts in enumerate(pc.OUT_SHIFTS_3):
            for tshift in (0, 5):
                run_offsets(t, docs, text, off, want, tshift, SUR_NAMES[(i + tshift) % 3], shifts, short, 8 * (i % 2), 8 * ((i // 2) % 2), ctx="variant %d" % variant)
    finally:
        t.variant(3)


# ------------------------------------------------------------------------------------------------
# c. what lies around the text does not matter
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sur", SUR_NAMES)
@pytest.mark.parametrize("mv", _params(2), ids=_id)
def test_c_surroundings_do_not_matter(tokenizer, mv, sur):
    """one small batch per END_CASE (each the last document of its own call, the end of the text at 0, 1, 7, 8, 9, 15 bytes past a multiple of 16 and
    of 512), the START_CASES first in turn, the adjacent pairs inside, at text shifts 0, 1, 8, 15: the ids form and the offsets form give the
    checker's answer for the payload.  The cases prove on the CPU checker that they would notice a neighbouring byte (pointer_cases.prove)."""
    model, variant = mv
    t = tokenizer(model)
    if sur == "completing":
        assert pc.prove(lambda b: tuple(x.tobytes() for x in t.offsets_of(b))) > 700 and pc.prove(lambda b: t.ids_of(b).tobytes()) > 700
    t.variant(variant)
    try:
        for k, (name, docs) in enumerate(pc.edge_batches()):
            text, off = flat_cases.pack(docs)
            want_i, want_o = t.want_ids(docs), t.want_offsets(docs)
            for tshift in (0, 1, 8, 15):
                ctx = "variant %d, case %s," % (variant, name)
                run_ids(t, docs, text, off, want_i, tshift, sur, 8 * (k % 2), (k + tshift) % 4, 8 * ((k // 2) % 2), ctx=ctx)
                run_offsets(t, docs, text, off, want_o, tshift, sur, pc.OUT_SHIFTS_3[(k + tshift) % 16], 0, 8 * ((k // 2) % 2), 8 * (k % 2), ctx=ctx)
    finally:
        t.variant(3)


# ------------------------------------------------------------------------------------------------
# d. the secondary Device calls
# ------------------------------------------------------------------------------------------------
def secondary_call(fn, pre, n, dtype, want, want_off, out_shift, ooff_shift, post=(), cap=None, null=False, what=""):
    """one Device call with its output at item shift out_shift and its offsets at byte shift ooff_shift: rc 0, complete offsets, the items that end at
    or before cap exact, nothing in front of the output or at / behind cap"""
    T, cap = int(want_off[-1]), int(want_off[-1]) if cap is None else cap
    out = pc.room(dtype, T, out_shift)
    ooff = pc.room(np.int64, n + 1, ooff_shift // 8)
    rc = fn(*pre, None if null else out.addr, cap, ooff.addr, *post, cur_stream())
    sync_stream()
    what = "%s, output +%d items, offsets +%d bytes, cap %d of %d%s" % (what, out_shift, ooff_shift, cap, T, ", NULL output" if null else "")
    assert rc == 0, (what, rc)
    g_off = ooff.fetch().result()
    if not np.array_equal(g_off, want_off):
        bad = int(np.nonzero(np.diff(g_off) != np.diff(want_off))[0][0]) if g_off[0] == 0 else -1
        raise AssertionError("%s: item %d: output size %d, expected %d" % (what, bad, g_off[bad + 1] - g_off[bad], want_off[bad + 1] - want_off[bad]))
    ooff.untouched(n + 1, what + ", offsets")
    if null:
        out.untouched(0, what)
        return
    done = T if cap >= T else int(want_off[np.searchsorted(want_off, cap, side="right") - 1])
    got = out.fetch().result()
    if not np.array_equal(got[:done], want[:done]):
        bad = int(np.nonzero(got[:done] != want[:done])[0][0])
        d = int(np.searchsorted(want_off, bad, side="right") - 1)
        raise AssertionError("%s: item %d differs at output position %d: got %r, expected %r" % (
            what, d, bad - int(want_off[d]), got[want_off[d]:want_off[d + 1]][:64].tolist(), want[want_off[d]:want_off[d + 1]][:64].tolist()))
    out.untouched(min(cap, T), what)


def long_text_docs():
    """three documents of more than 2,048 bytes with multi-byte characters across the 512-byte pieces (k_prep_wp_long, k_w2t_copy_long)"""
    a = ("д好x. Ünï çødé　text! " * 160).encode()
    b = b"a" + ("é" * 1400).encode() + " end. Then 好的。 one more sentence, here!".encode()
    c = b"xy " + ("好的。 Sentence two! Ünï çødé　" * 120).encode() + b"the end."
    assert min(len(a), len(b), len(c)) > 2048
    return [a, b, c]


@pytest.fixture(scope="module")
def text_docs():
    longs = long_text_docs()
    docs = sc.mixed_docs(301)
    docs.insert(40, longs[0])
    docs.insert(200, longs[1])
    docs.append(longs[2])                                      # the last document is a long one: the end of the text is inside its last piece
    return docs


@pytest.mark.parametrize("model,mode", [(None, 1), ("wbd.bin", 1), (None, 2), ("sbd.bin", 2)], ids=["words-builtin", "words-wbd", "sentences-builtin", "sentences-sbd"])
def test_d_words_and_sentences(text_docs, model, mode):
    import blingfire_amd as bf
    L = bf.lib()
    ck = sc.Checker()
    h = bf.load_model(bfutil.model_path(model)) if model else None
    hck = ck.load(model) if model else None
    try:
        fn_ck = ck.words if mode == 1 else ck.sentences
        fn = L.TextToWordsBatchDevice if mode == 1 else L.TextToSentencesBatchDevice
        text, off = sc.pack(text_docs)
        want, want_off = sc.pack([fn_ck(b, hck) for b in text_docs])
        n, T = len(text_docs), int(want_off[-1])
        assert want_off[-1] - want_off[-2] > 2048
        combos = [(ts, s) for ts in pc.TEXT_SHIFTS[::3] for s in ("completing", "invalid")]
        for i in range(36):                                    # every (text shift, surrounding) twice and more, every output shift 0 .. 17 twice
            tshift, sur = combos[i % len(combos)]
            ptext = pc.place(text, tshift, *SUR[sur])
            poff = pc.place(off, 8 * (i % 2), b"\xff", b"\xff")
            what = "%s %s, text +%d in '%s', doc offsets +%d" % ("TextToWords" if mode == 1 else "TextToSentences", model, tshift, sur, 8 * (i % 2))
            pre = [VP(h) if h else None, ptext.addr, poff.addr, n, len(text)]
            kw = {}
            if i == 7:
                kw = dict(null=True, cap=0)                                          # the size query
            elif i == 11:
                kw = dict(cap=int(want_off[-2]) + int(want_off[-1] - want_off[-2]) // 2)      # a text_cap inside the last document
            secondary_call(fn, pre, n, np.uint8, want, want_off, i % 18, 8 * ((i // 2) % 2), what=what, **kw)
            ptext.verify(what + ", text")
            poff.verify(what + ", doc offsets")
    finally:
        if h:
            bf.free_model(h)
        if hck:
            ck.free(hck)


def test_d_word_hyphenation():
    """the edge words of tests/test_w2h.py (stored reference answers), the last one ending with a truncated character, text and output at byte
    shifts 0 .. 8 each"""
    import blingfire_amd as bf
    import w2h_cases as wc
    named = wc.edge_words()
    words = [w for _, w in named]
    texts = wc.ref_texts("edge", wc.FIXTURE, words, wc.UHYS)["45"]
    order = [k for k, (name, _) in enumerate(named) if name != "truncated_3"] + [k for k, (name, _) in enumerate(named) if name == "truncated_3"]
    words, texts = [words[k] for k in order], [texts[k] for k in order]
    assert words[-1] == b"abc\xe2\x82"
    text, off = sc.pack(words)
    want, want_off = wc.pack_texts(texts)
    L = bf.lib()
    h = bf.load_model(wc.FIXTURE)
    try:
        for tshift in range(9):
            for oshift in range(9):
                i = 9 * tshift + oshift
                sur = SUR_NAMES[i % 3]
                ptext = pc.place(text, tshift, *SUR[sur])
                poff = pc.place(off, 8 * (i % 2), b"\xff", b"\xff")
                what = "WordHyphenation, text +%d in '%s'" % (tshift, sur)
                secondary_call(L.WordHyphenationBatchDevice, [VP(h), ptext.addr, poff.addr, len(words), len(text)], len(words), np.uint8, want, want_off, oshift,
                               8 * ((i // 2) % 2), post=[0x2D], what=what)
                ptext.verify(what + ", text")
                poff.verify(what + ", word offsets")
    finally:
        bf.free_model(h)


@pytest.mark.parametrize("model", ["gpt2.i2w", "xlnet.i2w"])
def test_d_ids_to_text(model):
    """d_ids at item shifts 0 .. 3 between in-range ids (an id taken in from the guard shows as text), text_out at byte shifts 0 .. 17"""
    import blingfire_amd as bf
    L = bf.lib()
    ck = sc.Checker()
    ntok = sc.i2w_count(model)
    h, hck = bf.load_model(bfutil.model_path(model)), ck.load(model)
    try:
        named = sc.i2t_sequences(sc.i2w_specials(ck, hck, ntok), ntok)
        seqs = [s for _, s in named]
        ids, off = sc.pack(seqs, np.int32)
        guard = np.array([1000], dtype=np.int32).tobytes()
        assert ck.ids_to_text(hck, [1000], 0) != b""
        for skip in (0, 1):
            want, want_off = sc.pack([ck.ids_to_text(hck, s, skip) for s in seqs])
            for oshift in range(18):
                i = oshift + 18 * skip
                pids = pc.place(ids, 4 * (i % 4), guard, guard)
                poff = pc.place(off, 8 * ((i // 4) % 2), b"\xff", b"\xff")
                what = "IdsToText %s skip_special=%d, ids +%d items, id offsets +%d" % (model, skip, i % 4, 8 * ((i // 4) % 2))
                secondary_call(L.IdsToTextBatchDevice, [VP(h), pids.addr, poff.addr, len(seqs)], len(seqs), np.uint8, want, want_off, oshift, 8 * ((i // 2) % 2),
                               post=[skip], what=what)
                pids.verify(what + ", ids")
                poff.verify(what + ", id offsets")
    finally:
        bf.free_model(h)
        ck.free(hck)


def test_d_dict_get_info():
    """d_keys, d_values_out, d_ret_out and d_info_ids_out at item shifts 0 .. 3, rotated independently; the keys lie between symbols of the
    dictionary's alphabet (a symbol taken in from the guard makes another key)"""
    import blingfire_amd as bf
    L = bf.lib()
    model = "gpt2.bin"
    h, dck = bf.load_model(bfutil.model_path(model)), sc.DictChecker(model)
    try:
        keys = sc.dict_edge_keys(model, dck)
        flat, off = sc.pack([np.array(k, dtype=np.int32) for k in keys], np.int32)
        ret, info, vals, v_off = dck.batch(keys)
        n = len(keys)
        guard = np.array([97], dtype=np.int32).tobytes()
        seen = set()
        for i in range(16):
            ks, vs, rs, fs = i % 4, (i // 4 + i) % 4, (3 * i + 1) % 4, (i // 2 + 2) % 4
            seen |= {("k", ks), ("v", vs), ("r", rs), ("f", fs)}
            pkeys = pc.place(flat, 4 * ks, guard, guard)
            poff = pc.place(off, 8 * (i % 2), b"\xff", b"\xff")
            r_ret, r_info = pc.room(np.int32, n, rs), pc.room(np.int32, n, fs)
            what = "DictGetInfo %s, keys +%d, ret +%d, info ids +%d items, key offsets +%d bytes" % (model, ks, rs, fs, 8 * (i % 2))
            secondary_call(L.DictGetInfoBatchDevice, [VP(h), pkeys.addr, poff.addr, n, r_ret.addr, r_info.addr], n, np.int32, vals, v_off, vs, 8 * ((i // 2) % 2), what=what)
            assert np.array_equal(r_ret.fetch().result(), ret) and np.array_equal(r_info.fetch().result(), info), what
            r_ret.untouched(n, what + ", ret")
            r_info.untouched(n, what + ", info ids")
            pkeys.verify(what + ", keys")
            poff.verify(what + ", key offsets")
        assert len(seen) == 16
    finally:
        bf.free_model(h)
        dck.close()


def rows_call(h, pids, ids_len, poff, nseq, par, want, shifts, what):
    """IdsToRowsBatchDevice with rows / mask / row_seq / row_first at the item shifts `shifts` and rows_cap = the exact total"""
    import blingfire_amd as bf
    L_, cls_id, sep_id, stride, max_rows, pad_left = par
    total = len(want[2])
    rows, mask = pc.room(np.int32, total * L_, shifts[0]), pc.room(np.uint8, total * L_, shifts[1])
    seq, first = pc.room(np.int32, total, shifts[2]), pc.room(np.int32, total, shifts[3])
    r_off = pc.room(np.int64, nseq + 1, shifts[4])
    r = bf.lib().IdsToRowsBatchDevice(VP(h), pids if isinstance(pids, int) else pids.addr, ids_len, poff if isinstance(poff, int) else poff.addr, nseq, L_, cls_id, sep_id,
                                      rc.PAD, stride, max_rows, 1 if pad_left else 0, rows.addr, mask.addr, seq.addr, first.addr, total, r_off.addr, cur_stream())
    sync_stream()
    assert r == 0, (what, r)
    assert bf.lib().BfLastStatus(VP(h)) == want[5], what
    assert np.array_equal(r_off.fetch().result(), want[4]), what
    for name, o, w, width in (("rows", rows, want[0], L_), ("mask", mask, want[1], L_), ("row_seq", seq, want[2], 1), ("row_first", first, want[3], 1)):
        g = o.fetch().result()
        if not np.array_equal(g, w.reshape(-1)):
            bad = int(np.nonzero(g != w.reshape(-1))[0][0])
            raise AssertionError("%s: %s differ in row %d, column %d: %d, expected %d" % (what, name, bad // width, bad % width, g[bad], w.reshape(-1)[bad]))
        o.untouched(total * width, what + ", " + name)
    r_off.untouched(nseq + 1, what + ", row offsets")


@pytest.mark.parametrize("L_", [64, 63, 8])
def test_d_ids_to_rows(L_):
    """d_ids at item shifts 0 .. 3 with ids_len = the exact total between in-range ids (an id taken in from the guard shows in a row), d_id_offsets
    at +0 / +8 bytes, every output at item shifts 0 .. 3"""
    import blingfire_amd as bf
    import test_gpu_rows
    h = bf.load_model(bfutil.model_path(bfutil.bert_model_name()))
    try:
        guard = np.array([7777], dtype=np.int32).tobytes()
        for par in ((L_, rc.CLS, rc.SEP, 1 if L_ > 8 else 2, 0, False), (L_, rc.CLS, -1, 0, 1, True)):
            for ids, off in (rc.synthetic(*rc.geometry(par[0], par[1], par[2], par[3])), test_gpu_rows.mixed(1500, 5, longest=3 * L_)):
                want = rc.restate(ids, off, par[0], par[1], par[2], rc.PAD, par[3], par[4], par[5])
                assert want[5] == 0
                for i in range(8):
                    pids = pc.place(ids, 4 * (i % 4), guard, guard)
                    poff = pc.place(off, 8 * ((i // 2) % 2), b"\xff", b"\xff")
                    shifts = ((i + 1) % 4, (5 * i) % 18, (i // 2) % 4, (3 * i + 2) % 4, i % 2)
                    what = "IdsToRows L %d, ids +%d items, id offsets +%d bytes, outputs +%s" % (L_, i % 4, 8 * ((i // 2) % 2), list(shifts))
                    rows_call(h, pids, len(ids), poff, len(off) - 1, par, want, shifts, what)
                    pids.verify(what + ", ids")
                    poff.verify(what + ", id offsets")
    finally:
        bf.free_model(h)


# ------------------------------------------------------------------------------------------------
# e. the chain the README describes: the tokenizer's outputs straight into rows
# ------------------------------------------------------------------------------------------------
def test_e_tokenizer_output_straight_into_rows(tokenizer):
    """TextToIdsBatchDevice with d_ids_out one item and d_id_offsets_out 8 bytes behind a 16-byte boundary, IdsToRowsBatchDevice on those addresses
    behind it on the same stream: 3,000 documents of config 2, L = 64, against the restatement over the checker's ids"""
    t = tokenizer("bert_base_tok.bin")
    text, off = bfutil.gen_workload("config2", 3000)
    docs = flat_cases.docs_of((text, off))
    wids, woff = t.want_ids(docs)
    nd, total = len(docs), int(woff[-1])
    want = rc.restate_truncated(wids, woff, 64, rc.CLS, rc.SEP, rc.PAD) + (0,)
    ptext = pc.place(text, 3, *SUR["completing"])
    poff = pc.place(off, 8, b"\xff", b"\xff")
    ids = pc.room(np.int32, total, 1)
    ido = pc.room(np.int64, nd + 1, 1)
    r = t.L.TextToIdsBatchDevice(VP(t.h), ptext.addr, poff.addr, nd, len(text), ids.addr, total, ido.addr, t.max_ids, t.unk, cur_stream())
    assert r == 0
    rows_call(t.h, ids.addr, total, ido.addr, nd, (64, rc.CLS, rc.SEP, 0, 1, False), want, (2, 3, 1, 3, 1), "tokenizer -> rows")
    assert np.array_equal(ido.fetch().result(), woff) and np.array_equal(ids.fetch().result(), wids)
    ids.untouched(total, "tokenizer -> rows, ids")
    ido.untouched(nd + 1, "tokenizer -> rows, id offsets")
    ptext.verify("tokenizer -> rows, text")
    poff.verify("tokenizer -> rows, doc offsets")
