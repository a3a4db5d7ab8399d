"""The secondary batch calls of the C-ABI -- IdsToTextBatch, NormalizeSpacesBatch, TextToHashesBatch, DictGetInfoBatch, TextToWordsBatch,
TextToSentencesBatch and the ...Device forms of four of them -- where their kernels get interesting:

  A  batches of more documents than the grid has waves (3 * 64 * CUs + 17: every wave of k_i2t_*, k_normsp, k_hash_*, k_w2t_*, k_s2t_* takes
     three documents or more and has to start each of them clean), of 300,007 documents (k_scan_top's carry loop runs twice) and, for the
     dictionary, of more keys than k_dict_* has lanes;
  B  the deterministic edge inputs of tests/secondary_cases.py: state carried from one 64-element window to the next (the first solid token of
     an id sequence in a late window, characters and white-space runs across a window edge, tokens and token counts beyond 64);
  C  the capacity contracts of include/blingfiretokdll_amd.h: the host forms answer BF_E_CAPACITY with complete offsets and leave the
     output alone, the Device forms fill only the offsets when the output pointer is NULL and never write at or past the capacity.  The
     Device output tensor is always allocated 4,096 items beyond the full size and pre-filled, so a write a guard should have stopped lands
     in memory this test owns and shows as a changed canary.

Every expectation is the unmodified reference's (oracle/_ref, bfutil.have_ref()), asked once per distinct document; the large batches repeat
and permute those documents with numpy (secondary_cases.tile), and the comparison is one array comparison.  Without oracle/_ref the oracle
restatement stands in, which tests/test_secondary_edges.py pins to the reference on the inputs of B.

Nothing is left out of a comparison, with one kind of input never given: a dictionary key with a negative symbol, on which the reference
itself reads out of bounds (FADictInterpreter_t.h:369-390 indexes the character map with it; tests/test_dict_lookup.py keys_for(negative=))."""
import ctypes

import numpy as np
import pytest

import bfutil
import secondary_cases as sc

pytestmark = pytest.mark.gpu

E_CAPACITY = -3
SLACK = 4096
CANARY = {np.dtype(np.uint8): 0xA5, np.dtype(np.int32): 0x5A5A5A5A}
I64, VP, CI = ctypes.c_int64, ctypes.c_void_p, ctypes.c_int


@pytest.fixture(scope="module")
def L():
    import blingfire_amd as bf
    lib = bf.lib()
    lib.NormalizeSpacesBatch.restype = lib.TextToHashesBatch.restype = I64
    lib.NormalizeSpacesBatch.argtypes = [VP, VP, I64, VP, I64, VP, CI]
    lib.TextToHashesBatch.argtypes = [VP, VP, I64, VP, I64, VP, CI, CI]
    return lib


@pytest.fixture(scope="module")
def ck():
    return sc.Checker()


@pytest.fixture(scope="module")
def cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _many(cus):
    """the two batch sizes of A: three documents or more for every wave of a grid of 16 * CUs blocks of 4; two rounds of k_scan_top"""
    return 3 * 64 * cus + 17, 300007


class Case:
    """One call on one batch.  host / dev: the entry points (dev None where the call has no Device form); pre / post: the arguments in
    front of (output, capacity, offsets) and behind them, as numpy arrays and plain values; total_bytes: the Device forms of
    TextToWords / TextToSentences take the input size; extras: further per-item outputs (DictGetInfo's ret and info ids) as
    (position in pre, expected)."""

    def __init__(self, what, host, dev, pre, post, n, want, want_off, items, total_bytes=None, extras=()):
        self.what, self.host, self.dev, self.pre, self.post, self.n = what, host, dev, pre, post, n
        self.want, self.want_off, self.items, self.total_bytes, self.extras = want, want_off, items, total_bytes, extras
        self.T = int(want_off[-1])
        self.names = None                                       # of the items, for the messages (the named inputs of secondary_cases)
        self._dev_pre = None

    # ---- host form
    def run_host(self, cap):
        out = np.full(max(self.T, cap, 0) + 64, CANARY[self.want.dtype], dtype=self.want.dtype)
        off = np.full(self.n + 1, -1, dtype=np.int64)
        pre = [a.ctypes.data if isinstance(a, np.ndarray) else a for a in self.pre]
        rc = self.host(*pre, out.ctypes.data, cap, off.ctypes.data, *self.post)
        return rc, out, off

    # ---- Device form
    def run_dev(self, cap, null_out=False, side_stream=False, stream=None):
        """stream: the torch stream to run on (a caller's own); else a fresh side stream or the current one"""
        import torch
        dev = torch.device("cuda:0")
        if self._dev_pre is None:
            self._dev_pre = [torch.from_numpy(a).to(dev) if isinstance(a, np.ndarray) else a for a in self.pre]
            torch.cuda.synchronize()
        if stream is None:
            stream = torch.cuda.Stream() if side_stream else torch.cuda.current_stream()
        tdt = torch.uint8 if self.want.dtype == np.uint8 else torch.int32
        with torch.cuda.stream(stream):
            out = torch.full((self.T + SLACK,), CANARY[self.want.dtype], dtype=tdt, device=dev)
            off = torch.full((self.n + 1,), -1, dtype=torch.int64, device=dev)
            for pos, _ in self.extras:
                self._dev_pre[pos].fill_(-77)
            pre = [a.data_ptr() if isinstance(a, torch.Tensor) else a for a in self._dev_pre]
            if self.total_bytes is not None:
                pre.append(self.total_bytes)
            rc = self.dev(*pre, None if null_out else out.data_ptr(), cap, off.data_ptr(), *self.post, VP(stream.cuda_stream))
        stream.synchronize()
        extras = [self._dev_pre[pos].cpu().numpy() for pos, _ in self.extras]
        return rc, out.cpu().numpy(), off.cpu().numpy(), extras

    # ---- comparisons
    def _offsets(self, off, how):
        assert np.array_equal(off, self.want_off), sc.first_difference(off, self.want_off, self.items, "%s, %s" % (self.what, how), self.names)

    def _exact(self, out, off, upto, how):
        """out[0 .. upto) is the expectation (upto = the end of the last item that is complete)"""
        if not np.array_equal(out[:upto], self.want[:upto]):
            bad = int(np.nonzero(out[:upto] != self.want[:upto])[0][0])
            d = int(np.searchsorted(self.want_off, bad, side="right") - 1)
            raise AssertionError("%s, %s: %s differs at output position %d: got %r, expected %r" % (
                self.what, how, sc.describe(self.items, d, self.names), bad - int(self.want_off[d]),
                out[self.want_off[d]:self.want_off[d + 1]][:64].tolist(), self.want[self.want_off[d]:self.want_off[d + 1]][:64].tolist()))

    def _untouched(self, out, frm, how):
        tail = out[frm:]
        assert (tail == CANARY[self.want.dtype]).all(), "%s, %s: output written at position %d, at or past the capacity / size %d" % (
            self.what, how, frm + int(np.nonzero(tail != CANARY[self.want.dtype])[0][0]), frm)

    def short_caps(self):
        """T - 1, T / 2, a capacity inside the largest item (not at an item boundary), 1"""
        T = self.T
        k = int(np.argmax(np.diff(self.want_off)))
        cut = int(self.want_off[k]) + max(1, int(self.want_off[k + 1] - self.want_off[k]) // 2)
        return [c for c in dict.fromkeys([T - 1, T // 2, cut, 1]) if 0 <= c < T]

    def check(self, capacity=True):
        T = self.T
        # host form, full size
        rc, out, off = self.run_host(T)
        if rc == E_CAPACITY or rc >= 0:
            self._offsets(off, "host")                          # (complete also with BF_E_CAPACITY: names the first item whose size is wrong)
        assert rc == T, "%s: the host form returned %d, %d expected" % (self.what, rc, T)
        self._exact(out, off, T, "host")
        self._untouched(out, T, "host")
        for pos, want in self.extras:
            assert np.array_equal(self.pre[pos], want), "%s: per-item result %d differs at item %d" % (self.what, pos, int(np.nonzero(self.pre[pos] != want)[0][0]))
        if T > 0:
            for cap in ([T - 1, T // 2, 0] if capacity else [T - 1]):
                rc, out, off = self.run_host(cap)
                assert rc == E_CAPACITY, "%s: capacity %d of %d: the host form returned %d" % (self.what, cap, T, rc)
                self._offsets(off, "host, capacity %d of %d" % (cap, T))
                self._untouched(out, 0, "host, capacity %d of %d" % (cap, T))
        if self.dev is None:
            return
        # Device form: size query, full size, short capacities
        rc, out, off, ex = self.run_dev(0, null_out=True)
        assert rc == 0
        self._offsets(off, "Device, NULL output")
        self._untouched(out, 0, "Device, NULL output")
        rc, out, off, ex = self.run_dev(T)
        assert rc == 0
        self._offsets(off, "Device")
        self._exact(out, off, T, "Device")
        self._untouched(out, T, "Device")
        for (pos, want), got in zip(self.extras, ex):
            assert np.array_equal(got, want), "%s, Device: per-item result %d differs at item %d" % (self.what, pos, int(np.nonzero(got != want)[0][0]))
        caps = self.short_caps() if capacity else [T // 2]
        for j, cap in enumerate(caps):
            how = "Device, capacity %d of %d" % (cap, T)
            rc, out, off, ex = self.run_dev(cap, side_stream=(j == len(caps) - 1 or j == 1))
            assert rc == 0, how
            self._offsets(off, how)
            done = int(self.want_off[np.searchsorted(self.want_off, cap, side="right") - 1])      # the last item boundary at or before cap
            self._exact(out, off, done, how)
            self._untouched(out, cap, how)


# ------------------------------------------------------------------------------------------------
# case builders: expectation per distinct item from the checker, then tiled
# ------------------------------------------------------------------------------------------------
def _tiled(flat, off, w_flat, w_off, idx):
    if idx is None:
        return flat, off, w_flat, w_off
    a, b = sc.tile(flat, off, idx)
    c, d = sc.tile(w_flat, w_off, idx)
    return a, b, c, d


def i2t_case(L, h, ck, hck, seqs, skip, idx=None, what="IdsToText"):
    flat, off = sc.pack(seqs, np.int32)
    w_flat, w_off = sc.pack([ck.ids_to_text(hck, s, skip) for s in seqs])
    flat, off, w_flat, w_off = _tiled(flat, off, w_flat, w_off, idx)
    n = len(off) - 1
    return Case("%s skip_special=%d, %d sequences" % (what, skip, n), L.IdsToTextBatch, L.IdsToTextBatchDevice, [VP(h), flat, off, n], [skip], n, w_flat, w_off, (flat, off))


def normsp_case(L, ck, docs, usp, idx=None):
    flat, off = sc.pack(docs)
    w_flat, w_off = sc.pack([ck.normalize(b, usp) for b in docs])
    flat, off, w_flat, w_off = _tiled(flat, off, w_flat, w_off, idx)
    n = len(off) - 1
    return Case("NormalizeSpaces uSpace=0x%x, %d documents" % (usp, n), L.NormalizeSpacesBatch, None, [flat, off, n], [usp], n, w_flat, w_off, (flat, off))


def hash_case(L, ck, docs, ngrams, bucket, idx=None):
    flat, off = sc.pack(docs)
    w_flat, w_off = sc.pack([ck.hashes(b, ngrams, bucket) for b in docs], np.int32)
    flat, off, w_flat, w_off = _tiled(flat, off, w_flat, w_off, idx)
    n = len(off) - 1
    return Case("TextToHashes ngrams=%d bucket=%d, %d documents" % (ngrams, bucket, n), L.TextToHashesBatch, None, [flat, off, n], [ngrams, bucket], n, w_flat, w_off, (flat, off))


def text_case(L, ck, docs, mode, h=None, hck=None, idx=None):
    flat, off = sc.pack(docs)
    fn = ck.words if mode == 1 else ck.sentences
    w_flat, w_off = sc.pack([fn(b, hck) for b in docs])
    flat, off, w_flat, w_off = _tiled(flat, off, w_flat, w_off, idx)
    n = len(off) - 1
    host, dev = (L.TextToWordsBatch, L.TextToWordsBatchDevice) if mode == 1 else (L.TextToSentencesBatch, L.TextToSentencesBatchDevice)
    return Case("%s, %d documents" % ("TextToWords" if mode == 1 else "TextToSentences", n), host, dev, [VP(h) if h else None, flat, off, n], [], n, w_flat, w_off,
                (flat, off), total_bytes=int(off[-1]))


def dict_case(L, h, dck, keys, idx=None, model=""):
    flat, off = sc.pack([np.array(k, dtype=np.int32) for k in keys], np.int32)
    ret, ids, vals, v_off = dck.batch(keys)
    if idx is not None:
        flat, off = sc.tile(flat, off, idx)
        vals, v_off = sc.tile(vals, v_off, idx)
        ret, ids = ret[idx], ids[idx]
    n = len(off) - 1
    return Case("DictGetInfo %s, %d keys" % (model, n), L.DictGetInfoBatch, L.DictGetInfoBatchDevice, [VP(h), flat, off, n, np.zeros(n, np.int32), np.zeros(n, np.int32)], [],
                n, vals, v_off, (flat, off), extras=[(4, ret), (5, ids)])


# ------------------------------------------------------------------------------------------------
# A. many documents
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mixed():
    return sc.mixed_docs(), sc.short_docs()


@pytest.mark.parametrize("skip", [0, 1])
def test_many_sequences_ids_to_text(L, ck, cus, skip):
    import blingfire_amd as bf
    model = "gpt2.i2w"
    ntok = sc.i2w_count(model)
    h, hck = bf.load_model(bfutil.model_path(model)), ck.load(model)
    try:
        for n, short in zip(_many(cus), (False, True)):
            seqs = sc.i2t_mixed(ntok, short=short)
            i2t_case(L, h, ck, hck, seqs, skip, sc.tiling(len(seqs), n, 41 + skip)).check(capacity=False)
    finally:
        bf.free_model(h)
        ck.free(hck)


@pytest.mark.parametrize("usp", [0x2581, 0x20])
def test_many_documents_normalize_spaces(L, ck, cus, mixed, usp):
    for n, docs in zip(_many(cus), mixed):
        normsp_case(L, ck, docs, usp, sc.tiling(len(docs), n, 43)).check(capacity=False)


@pytest.mark.parametrize("ngrams", [1, 3])
def test_many_documents_text_to_hashes(L, ck, cus, mixed, ngrams):
    for n, docs in zip(_many(cus), mixed):
        hash_case(L, ck, docs, ngrams, 2000000, sc.tiling(len(docs), n, 47)).check(capacity=False)


@pytest.mark.parametrize("mode", [1, 2])
def test_many_documents_words_and_sentences(L, ck, cus, mixed, mode):
    """the built-in models, host and Device forms"""
    for n, docs in zip(_many(cus), mixed):
        text_case(L, ck, docs, mode, idx=sc.tiling(len(docs), n, 53)).check(capacity=False)


@pytest.mark.parametrize("model", ["gpt2.bin", "xlm_roberta_base.bin"])
def test_many_keys_dict_get_info(L, cus, model):
    import blingfire_amd as bf
    import test_dict_lookup
    keys = test_dict_lookup.keys_for(model, n_random=3000, seed=3, negative=False)      # (negative symbols: see the module docstring)
    if len(keys) % 2 == 0:
        keys.append([0x2581, 97])
    h, dck = bf.load_model(bfutil.model_path(model)), sc.DictChecker(model)
    try:
        n = 16 * 256 * cus + 4099                                  # every lane of k_dict_ids / k_dict_fill takes a second key
        case = dict_case(L, h, dck, keys, sc.tiling(len(keys), n, 59), model)
        assert (np.diff(case.want_off) > 0).sum() > n // 20        # hits throughout
        case.check(capacity=False)
    finally:
        bf.free_model(h)
        dck.close()


# ------------------------------------------------------------------------------------------------
# B + C. long inputs, window edges, capacities
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", sc.I2W_MODELS)
def test_edges_ids_to_text(L, ck, model):
    import blingfire_amd as bf
    ntok = sc.i2w_count(model)
    h, hck = bf.load_model(bfutil.model_path(model)), ck.load(model)
    try:
        named = sc.i2t_sequences(sc.i2w_specials(ck, hck, ntok), ntok)
        for skip in (0, 1):
            case = i2t_case(L, h, ck, hck, [s for _, s in named], skip, what="IdsToText " + model)
            case.names = [n for n, _ in named]
            # a sequence with an unknown id has no text (unless skip_special leaves the id out), its neighbours have theirs
            for k, (name, _) in enumerate(named):
                if name.startswith("unknown_") and not skip:
                    assert case.want_off[k + 1] == case.want_off[k] and case.want_off[k] > case.want_off[k - 1] and case.want_off[k + 2] > case.want_off[k + 1]
            case.check()
    finally:
        bf.free_model(h)
        ck.free(hck)


@pytest.mark.parametrize("usp", sc.USPACES)
def test_edges_normalize_spaces(L, ck, usp):
    named = sc.normsp_docs()
    case = normsp_case(L, ck, [b for _, b in named], usp)
    case.names = [n for n, _ in named]
    assert usp == 0xD800 or case.T > 10000000
    case.check()
    # the single-document call on the documents with the most state to carry
    import blingfire_amd as bf
    for name, b in named:
        if name.endswith("features_64k") or "trailing_ws_200" in name or "lone_continuation" in name or "no_ws_then" in name:
            o = ctypes.create_string_buffer(b"\x7f" * (4 * len(b) + 16))
            r = bf.lib().NormalizeSpaces(b, len(b), o, 4 * len(b) + 16, usp)
            want = ck.normalize(b, usp)
            assert (o.raw[:r] if r > 0 else b"") == want, ("NormalizeSpaces", name, hex(usp), r, len(want))


def test_normalize_spaces_batch_with_a_uspace_that_cannot_be_encoded(L, ck):
    """found by test_edges_normalize_spaces[0xD800]: NormalizeSpaces fails on a document that needs a uSpace no UTF-8 sequence encodes
    (FAUtf8Utils.cpp:549-552), so in the batch form such a document yields nothing; k_normsp sized it as its text without the spaces.
    Documents that need none (no white space, or only leading and trailing white space) keep their text."""
    docs = [b"a b", b"ab", b"ab ", b" ab", b"a\tb c", b"  ", b"ab" * 100 + b" " * 70, b"x" * 63 + b" y", "é　好".encode()]
    case = normsp_case(L, ck, docs, 0xD800)
    assert np.diff(case.want_off).tolist() == [0, 2, 2, 2, 0, 0, 200, 0, 0]
    case.check()


@pytest.mark.parametrize("ngrams,bucket", sc.HASH_PARAMS)
def test_edges_text_to_hashes(L, ck, ngrams, bucket):
    named = sc.hash_docs()
    case = hash_case(L, ck, [b for _, b in named], ngrams, bucket)
    case.names = [n for n, _ in named]
    case.check()


@pytest.mark.parametrize("model", ["gpt2.bin", "xlm_roberta_base.bin"])
def test_edges_dict_get_info(L, model):
    import blingfire_amd as bf
    h, dck = bf.load_model(bfutil.model_path(model)), sc.DictChecker(model)
    try:
        case = dict_case(L, h, dck, sc.dict_edge_keys(model, dck), model=model)
        gaps = np.diff(case.want_off)
        assert (gaps == 0).sum() > 1000 and (gaps > 0).sum() > 1000
        case.check()
    finally:
        bf.free_model(h)
        dck.close()


@pytest.mark.parametrize("model,mode", [(None, 1), (None, 2), ("wbd.bin", 1), ("sbd.bin", 2)])
def test_capacity_words_and_sentences_long_documents(L, ck, model, mode):
    """documents of more than 1,024 tokens are assembled by k_w2t_copy_long, which has a capacity guard of its own: the largest document and
    the last one are such documents, so the capacities inside the largest and of T - 1 end in its stores.  After the short calls a full-size
    call on the same handle is exact again: the list of long documents (counted in the handle's status words) starts empty every time."""
    import blingfire_amd as bf
    import test_words
    long_docs = [b for b in test_words._long_docs(7) if len(b) > 4000]
    assert len(long_docs) >= 8
    docs = sc.mixed_docs(301)
    for k, b in enumerate(long_docs):
        docs.insert(17 + 23 * k, b)
    docs.append(b"One sentence here. And a second one, of a few words more. " * 700)
    h = bf.load_model(bfutil.model_path(model)) if model else None
    hck = ck.load(model) if model else None
    try:
        case = text_case(L, ck, docs, mode, h, hck)
        if mode == 1:
            assert case.want[case.want_off[-2]:].tobytes().count(b" ") > 1024
        case.check()
        rc, out, off, _ = case.run_dev(case.T)                 # ... and once more at full size, behind the short capacities of check()
        assert rc == 0
        case._offsets(off, "Device, after short capacities")
        case._exact(out, off, case.T, "Device, after short capacities")
        case._untouched(out, case.T, "Device, after short capacities")
        rc, out, off = case.run_host(case.T)
        assert rc == case.T
        case._exact(out, off, case.T, "host, after short capacities")
    finally:
        if h:
            bf.free_model(h)
        if hck:
            ck.free(hck)
