"""TEST helpers of tests/test_gpu_beyond_2gib.py (GPU tier) and tests/test_big_offset_cases_host.py (CPU tier): batches whose document offsets,
staging slots and workspace cells lie beyond 2^31 bytes, and one whose ids lie beyond 2^31 output cells -- what DESIGN.md's "everything is 64-bit"
promises and the headline workload (10 M documents of 512 bytes) needs.

    real documents   bfutil.ADVERSARIAL, 300 fuzz documents, one document of more than 2048 bytes (k_prep_wp_long) and one of more than 4096 (more
                     than 1024 tokens: w2t_list_long), an empty and a one-byte document, and -- the last bytes of the batch -- a document that
                     ends inside a three-byte character.  The expectation is the checker's (the compiled reference where oracle/_ref is built,
                     else the oracle), asked once per model and call.
    filler A         two documents of 2^30 bytes in front of the real ones.  Each is over the reference's limit of 10^9 bytes
                     (FALimits::MaxArrSize), which every entry point tests BEFORE it reads a byte or allocates (blingfiretokdll.cpp:198, 449, 835,
                     1121, 1362: the comparison is the first statement behind the test for an empty input): no ids, no words, no sentences, no
                     hyphenated word.  The kernels restate the rule per document, so the filler costs them nothing and still puts every real
                     document's byte offset, slot and workspace cell behind 2^31.
    filler B         512 documents of WF_DOC_MAX = 4 MiB of ASCII spaces, 2^31 bytes that a program really walks, no document too long for the
                     flat program.  WordPiece: no ids.  Unigram (xlm_roberta_base.bin): the dummy prefix alone, one id; the compiled reference
                     answers one such document in 0.06 s on the build machine (BERT: 0.14 s) and both Unigram forms walk the 2 GiB in 30 ms on
                     an MI355X (70 GB/s: 512 documents are 512 waves of k_prep_sp8; the flat WordPiece program takes 11 ms), so they are in.  Not for BPE
                     models: a long uniform run is the arc-pool case of tests/test_zz_gpu_bpe_arc_pool.py.
    batch C          N copies of one document of 255 one-letter words (512 bytes, 255 ids with every BERT model), N the smallest number
                     with N * 255 > 2^31 + 2^20: ids at output positions beyond 2^31, a document that straddles 2^31, int64 id offsets.

device_bytes() restates bf_capi.cpp's reserve_* formulas: what BfReserve allocates for a batch, plus the test's own text and outputs.  The
lane-per-document BPE kernels are NOT in the matrix, on purpose: reserve_sp_workspaces reserves about 100 bytes per stream element for them (96 for
the arc lists alone), 260 GB for 2 GiB of text -- more than the device has once the text and the other workspaces are counted.  That leaves out
TextToIdsWithOffsetsBatchDevice on a BPE model too (the offsets API of gpt2.bin and roberta.bin has no other road) and BfSetVariant's bit 0x40."""
import functools

import numpy as np

import bfutil

GIB = 1 << 30
TWO31 = 1 << 31
LIMIT = 1000000000                          # FALimits::MaxArrSize
WF_DOC_MAX = 1 << 22                        # bf_flat_key.h
FILLER_A = (GIB, GIB)                       # bytes of the two documents
FILLER_B_DOCS = TWO31 // WF_DOC_MAX         # 512
GUARD = 64
MAX_IDS = 8192                              # more than any real document has ids
UNK = {"wp": 100, "unigram": 3, "bpe": 0}

# model -> (family, stream elements per byte of the _sp slots, bytes of a Unigram record, BPE wave program); tests/test_big_offset_cases_host.py
# holds the table to what the loader says of each model (tests/hosttest bft_reserve_facts)
FACTS = {
    "bert": ("wp", 1, 0, 0),
    "xlm_roberta_base.bin": ("unigram", 2, 4, 0),
    "xlnet.bin": ("unigram", 2, 4, 0),
    "gpt2.bin": ("bpe", 1, 0, 1),
    "roberta.bin": ("bpe", 1, 0, 1),
}


def model_file(model):
    return bfutil.bert_model_name() if model == "bert" else model


def family(model):
    return FACTS[model][0]


# ------------------------------------------------------------------------------------------------
# real documents
# ------------------------------------------------------------------------------------------------
TRUNCATED_TAIL = b"the last bytes of the batch end inside a character \xe2\x82"


@functools.lru_cache(maxsize=None)
def real_docs():
    """the same bytes for every model and call"""
    import reserve_cases
    long_2k = reserve_cases._words_text(2500, 7)                                # > 2048 bytes: k_prep_wp_long
    long_4k = b" ".join(reserve_cases.SHORT_WORDS * 120)[:4700]                 # > 4096 bytes, about 1,900 tokens: w2t_list_long (more than 1024 tokens)
    docs = list(bfutil.ADVERSARIAL) + bfutil.fuzz_docs(300, seed=31) + [long_2k, b"", long_4k, b"x", b"", TRUNCATED_TAIL]
    return tuple(docs)


def pack(docs):
    off = np.zeros(len(docs) + 1, dtype=np.int64)
    np.cumsum([len(d) for d in docs], out=off[1:])
    return np.frombuffer(b"".join(docs), dtype=np.uint8).copy(), off


def checker():
    return bfutil.reference() if bfutil.have_ref() else bfutil.oracle()


@functools.lru_cache(maxsize=None)
def expected_ids(model):
    """(ids, id offsets) of TextToIds per real document"""
    ck = checker()
    h = ck.load(bfutil.model_path(model_file(model)))
    try:
        text, off = pack(real_docs())
        ids, id_off = ck.batch(h, text, off, MAX_IDS, UNK[family(model)])
    finally:
        ck.free(h)
    ids.setflags(write=False); id_off.setflags(write=False)
    return ids, id_off


@functools.lru_cache(maxsize=None)
def expected_offsets(model):
    """(ids, first bytes, last bytes, id offsets) of TextToIdsWithOffsets per real document"""
    ck = checker()
    name = "TextToIdsWithOffsets" if bfutil.have_ref() else "bfo_text_to_ids_with_offsets"
    h = ck.load(bfutil.model_path(model_file(model)))
    try:
        wi, ws, we = [], [], []
        docs = real_docs()
        id_off = np.zeros(len(docs) + 1, dtype=np.int64)
        for d, b in enumerate(docs):
            c, i_, s_, e_ = ck.with_offsets(h, b, min(MAX_IDS, len(b) + 1), UNK[family(model)], name)
            wi.append(np.asarray(i_, dtype=np.int32)); ws.append(np.asarray(s_, dtype=np.int32)); we.append(np.asarray(e_, dtype=np.int32))
            id_off[d + 1] = id_off[d] + c
    finally:
        ck.free(h)
    out = tuple(np.concatenate(x) for x in (wi, ws, we)) + (id_off,)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def expected_text(mode):
    """(bytes, offsets) of TextToWords (mode 1) / TextToSentences (2) with the built-in model per real document"""
    import secondary_cases as sc
    ck = sc.Checker()
    fn = ck.words if mode == 1 else ck.sentences
    flat, off = pack([fn(b) for b in real_docs()])
    flat.setflags(write=False); off.setflags(write=False)
    return flat, off


def hyphenation_words():
    import w2h_cases as wc
    return [w for _, w in wc.edge_words()]


@functools.lru_cache(maxsize=None)
def expected_hyphenation():
    """(bytes, offsets) of WordHyphenationWithModel (uHy = '-') per word of w2h_cases.edge_words(): the stored answers of tests/test_w2h.py"""
    import w2h_cases as wc
    texts = wc.ref_texts("edge", wc.FIXTURE, hyphenation_words(), wc.UHYS)["45"]
    flat, off = wc.pack_texts(texts)
    flat = flat.copy(); flat.setflags(write=False); off.setflags(write=False)
    return flat, off


# ------------------------------------------------------------------------------------------------
# batches: the fillers in front of the items (documents or words)
# ------------------------------------------------------------------------------------------------
def filler_lengths(filler):
    return list(FILLER_A) if filler == "A" else [WF_DOC_MAX] * FILLER_B_DOCS


def batch_offsets(filler, items=None):
    """int64 offsets of filler + items (the real documents when None), and the number of filler documents"""
    fl = filler_lengths(filler)
    lens = fl + [len(d) for d in (real_docs() if items is None else items)]
    off = np.zeros(len(lens) + 1, dtype=np.int64)
    np.cumsum(lens, out=off[1:])
    return off, len(fl)


FILLER_B_IDS = {"wp": 0, "unigram": 1}      # ids of one filler B document: nothing; the dummy prefix alone


@functools.lru_cache(maxsize=None)
def filler_b_id(model):
    """the one id a Unigram model gives a document of spaces"""
    ck = checker()
    h = ck.load(bfutil.model_path(model_file(model)))
    try:
        c, buf = ck.text_to_ids(h, b" ", 4, UNK[family(model)])
    finally:
        ck.free(h)
    assert c == 1
    return buf[0]


def with_filler(want_off, nfill, per_filler=0):
    """output offsets of a batch from those of its items: every filler document has per_filler items in front"""
    head = np.arange(nfill + 1, dtype=np.int64) * per_filler
    return np.concatenate([head, want_off[1:] + head[-1]])


# ------------------------------------------------------------------------------------------------
# batch C
# ------------------------------------------------------------------------------------------------
C_WORDS = 255
C_DOC = (b" ".join(bytes([97 + i % 26]) for i in range(C_WORDS)) + b"   ")
C_MIN_IDS = TWO31 + (1 << 20)


def batch_c(k):
    """k = ids of the one document -> dict(ndocs, total_bytes, total_ids, straddler: the document with ids on both sides of output position 2^31)"""
    n = C_MIN_IDS // k + 1
    return dict(ndocs=n, total_bytes=n * len(C_DOC), total_ids=n * k, straddler=TWO31 // k if TWO31 % k else None)


def batch_c_capped(k, cap):
    """what a call with ids_cap = cap owes: (documents wholly below the cap, ids below the cap)"""
    whole = cap // k
    return whole, min(cap, batch_c(k)["total_ids"])


# ------------------------------------------------------------------------------------------------
# device memory (bf_capi.cpp restated: a size that changes there has to change here)
# ------------------------------------------------------------------------------------------------
def _buf(n):
    """DevBuf::reserve: an eighth more than asked, and 256 bytes"""
    return n + n // 8 + 256 if n > 0 else 0


def _merge(into, more):
    for k, v in more.items():
        into[k] = max(into.get(k, 0), v)


def _ids_workspaces(facts, D, B, want_off, variant, words=0):
    """reserve_ids_workspaces without the long-document workspace of the words modes: buffer -> bytes asked"""
    fam, mul, uni_rec, bpe_wave = facts
    w = dict(nchars=(D + 1) * 4, counts=(D + 1) * 4, bsums=((D + 1023) // 1024 + 1) * 8, tmp=(B + 8 * D + 64) * 4)
    if fam != "wp":                                             # reserve_sp_workspaces
        cap = mul * (B + D) + 64
        _merge(w, dict(cls=cap * 2 + 512, tmp=cap * 4, perm=(D + 1) * 4, hist=2048 * 4, narcs=(D + 1) * 4))
        if want_off:
            _merge(w, dict(srcoff=cap * 4, span=cap * 8))
        if fam == "unigram":
            w["s1"] = cap * uni_rec + 256
        elif bpe_wave and not want_off and not (variant & 0x40):
            _merge(w, dict(s1=cap * 24 + 256, big=64 << 20, bwflags=(D + 1) * 4))
        else:                                                   # the lane-per-document BPE kernels: not in the matrix (module docstring)
            bm = (cap >> 5) + D + 4
            _merge(w, dict(s1=(6 * cap + 32 * D + 64) * 16, s2=max(cap * 4, 2 * bm * 4) + (D + 16) * 4, s3=cap * 4, s4=cap, big=64 << 20))
        return w
    low = variant & 0xFF
    wave = not words and low != 2
    flat = wave and D > 0 and (low == 4 or (low == 3 and D >= 1024 and B >= (1 << 20)))
    if flat:                                                    # reserve_flat_workspaces (nranges <= D)
        nr = max(1, min(D, max(B // 16384 + 1, B // WF_DOC_MAX + 1)))
        _merge(w, dict(ent=(B + 64) * 4, home=(B + 64) * 4, entoff=(D + 1) * 8, entcnt=(D + 1) * 4, dstat=(D + 1) * 4, list=(D + 1) * 4, ranges=(nr + 2) * 8,
                       wrec=((B >> 4) + 64) * 16 + (nr + 2) * 8))
        if want_off:
            _merge(w, dict(espan=(B + 64) * 4, hspan=(B + 64) * 8, chard=(D + 1) * 4))
    if wave:
        if want_off:
            w["span"] = (B + 8 * D + 64) * 8
        return w
    _merge(w, dict(cls=(B + 64) * 2, flags=((B >> 10) + 2) * 8, preplong=(B // 2048 + 1) * 8))      # reserve_lane_lexer_workspaces
    if want_off:
        _merge(w, dict(srcoff=(B + 64) * 4, span=(B + 8 * D + 64) * 8))
    return w


def _long_workspace(B, D):
    """long_caps(): w_long of a words call (BfReserve leaves it out; the call allocates it, counted apart by BfWorkspaceGrows)"""
    thresh = min(max(16, B // 24000), 1 << 30)
    docs = min(D, B // (thresh + 1)) + 1
    chunks = min(B // 64 + 2 * docs + 1, 2 << 20)
    spec = (docs * 16 + 255) & ~255                             # (LexLongDoc: 16 bytes)
    return spec + chunks * (64 * 16 * 2 + 64 * 8 + 16) + (chunks * (64 * 16 + 16) if B + 1 > (1 << 19) else 0)


def reserved_bytes(model, D, B, want_off, variant=3, call="ids"):
    """what BfReserve(h, D, B, want_off) allocates on a fresh handle of `model` with BfSetVariant(variant), and a words call's w_long"""
    facts = FACTS[model] if model in FACTS else ("w2h", 1, 0, 0)
    w = dict(counts=(D + 1) * 4, bsums=((D + 1023) // 1024 + 1) * 8, rowseq=(D + 1) * 4, rowfirst=(D + 1) * 4)      # reserve_rows_workspaces
    n = D + 2                                                   # reserve_packed_workspaces
    _merge(w, dict(counts=n * 4, pkW=n * 8, pkjmp0=n * 4, pkjmp1=n * 4, pkmark=n * 4, pkmoff=n * 8, pkf=n * 4))
    n = (B + 63) // 64 + 2                                      # reserve_charpos_workspaces
    _merge(w, dict(cplead=n * 8, cpfour=n * 8, cpcnt=n * 4, cpP=n * 8))
    if facts[0] == "w2h":                                       # reserve_w2h_workspaces: documents = words
        _merge(w, dict(hcls=(B + 2 * D + 64) * 2, hnch=(D + 1) * 4, hsrc=(D + 1) * 4))
    else:
        _merge(w, _ids_workspaces(facts, D, B, False, variant))
        if want_off:
            _merge(w, _ids_workspaces(facts, D, B, True, variant))
        if facts[0] == "wp":                                    # the words modes of a WordPiece handle, and reserve_words_workspaces
            _merge(w, _ids_workspaces(facts, D, B, True, variant, words=1))
            _merge(w, dict(w2tlong=(B // 1024 + 2) * 8, ids=(B + 1) * 4, starts=(B + 1) * 4, ends=(B + 1) * 4, idoff=(D + 1) * 8))
    total = sum(_buf(v) for v in w.values())
    if call == "text":
        total += _buf(_long_workspace(B, D))
    return total + (256 << 20)                                  # the model's tables, the BPE arc pool and the handle's small blocks: below 256 MiB for every model here


def device_bytes(model, D, B, want_off, variant=3, call="ids", out_cells=0, out_arrays=1):
    """device memory of one test: the text and the document offsets, the outputs with their guards (out_arrays int32 arrays of out_cells, or one
    byte array for call="text"), the output offsets, and what the library reserves"""
    outs = (out_cells + GUARD) * (1 if call == "text" else 4 * out_arrays)
    return B + 48 + (D + 1) * 8 * 2 + outs + reserved_bytes(model, D, B, want_off, variant, call)


def enough_memory(need, free):
    """the only skip condition of the GPU tests: the device's free memory is below the need plus 10 %"""
    return free >= need + need // 10
