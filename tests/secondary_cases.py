"""Shared TEST helpers for the secondary batch calls (IdsToText, NormalizeSpaces, TextToHashes, DictGetInfo, TextToWords / TextToSentences):
the checker (the compiled reference where oracle/_ref is built, else the oracle restatement), the deterministic edge inputs of
tests/test_secondary_edges.py (CPU tier) and tests/test_gpu_secondary_at_scale.py (GPU tier) -- one builder, so both tiers see the same
bytes -- and the numpy tiling that turns a few thousand checked documents into batches of hundreds of thousands."""
import ctypes
import hashlib
import os

import numpy as np

import bfutil

VP, CI = ctypes.c_void_p, ctypes.c_int
DICTREF = os.path.join(bfutil.ROOT, "oracle", "_ref", "libdictref.so")
BOM = b"\xef\xbb\xbf"
USPACES = (0x2581, 0x20, ord("_"), 0x3000, 0x1F600, 0xD800)          # 0xD800 cannot be encoded: a document that needs one is rejected
HASH_PARAMS = [(ng, bucket) for ng in (1, 2, 3, 4) for bucket in (2000000, 7, -3)]     # never bucket 0: tokdll:710 divides by it
I2W_MODELS = ["gpt2.i2w", "xlnet.i2w", "bert_base_cased_tok.i2w"]


# ------------------------------------------------------------------------------------------------
# checker
# ------------------------------------------------------------------------------------------------
class Checker:
    """Per-document answers of the reference's own entry points (use_ref) or of their restatement in oracle/bf_oracle.c.
    Every method returns what the batch form owes for that document: the bytes / hashes without terminator, nothing where the
    single call fails."""

    def __init__(self, use_ref=None):
        self.is_ref = bfutil.have_ref() if use_ref is None else use_ref
        self.t = bfutil.reference() if self.is_ref else bfutil.oracle()
        L = self.t.lib
        if self.is_ref:
            self._ns, self._th, self._i2t = L.NormalizeSpaces, L.TextToHashes, L.IdsToText
            self._i2t.argtypes = [VP, VP, CI, VP, CI, ctypes.c_bool]
            self._w, self._s = L.TextToWordsWithModel, L.TextToSentencesWithModel
            self._w.argtypes = self._s.argtypes = [ctypes.c_char_p, CI, VP, CI, VP]
        else:
            self._ns, self._th, self._i2t = L.bfo_normalize_spaces, L.bfo_text_to_hashes, L.bfo_ids_to_text
            self._i2t.argtypes = [VP, VP, CI, VP, CI, CI]
            self._w, self._s = L.bfo_text_to_words_with_offsets, L.bfo_text_to_sentences_with_offsets
            self._w.argtypes = self._s.argtypes = [VP, ctypes.c_char_p, CI, VP, VP, VP, CI]
        self._ns.argtypes = [ctypes.c_char_p, CI, VP, CI, CI]
        self._th.argtypes = [ctypes.c_char_p, CI, VP, CI, CI, CI]
        for f in (self._ns, self._th, self._i2t, self._w, self._s):
            f.restype = CI
        self._builtin = {}

    def load(self, name):
        return self.t.load(bfutil.model_path(name))

    def free(self, h):
        self.t.free(h)

    def normalize(self, b, usp):
        cap = 4 * len(b) + 16
        o = ctypes.create_string_buffer(cap)
        r = self._ns(b, len(b), o, cap, usp)
        return o.raw[:r] if r > 0 else b""

    def hashes(self, b, ngrams, bucket):
        cap = (b.count(b" ") + 1) * ngrams + 1                 # tokdll:795: tokens * ngrams must stay below the capacity
        a = np.zeros(cap, dtype=np.int32)
        r = self._th(b, len(b), a.ctypes.data, cap, ngrams, bucket)
        assert r == cap - 1, ("TextToHashes of the checker", r, cap - 1, b[:40])
        return a[:r].copy()

    def ids_to_text(self, h, ids, skip):
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        arg = bool(skip) if self.is_ref else int(skip)
        r = self._i2t(VP(h), ids.ctypes.data, len(ids), None, 0, arg)      # capacity 0: nothing is written, the length comes back (tokdll:1731-1744)
        if r <= 1:
            return b""
        o = ctypes.create_string_buffer(r)
        assert self._i2t(VP(h), ids.ctypes.data, len(ids), o, r, arg) == r
        return o.raw[:r - 1]

    def _text(self, fn, b, h, default):
        cap = 4 * len(b) + 8
        o = ctypes.create_string_buffer(cap)
        if self.is_ref:
            r = fn(b, len(b), o, cap, VP(h) if h else None)     # NULL = the reference's built-in model
        else:
            if not h:
                if default not in self._builtin:
                    self._builtin[default] = self.load(default)
                h = self._builtin[default]
            r = fn(VP(h), b, len(b), o, None, None, cap)
        return o.raw[:r - 1] if r > 0 else b""

    def words(self, b, h=None):
        return self._text(self._w, b, h, "wbd.bin")

    def sentences(self, b, h=None):
        return self._text(self._s, b, h, "sbd.bin")


class DictChecker:
    """FADictInterpreter_t<int>::GetInfo of one model: oracle/_ref/libdictref.so (the reference's own interpreter) or the oracle."""
    MAX_OUT = 16

    def __init__(self, model, use_ref=None):
        self.is_ref = os.path.exists(DICTREF) if use_ref is None else use_ref
        path = bfutil.model_path(model).encode()
        if self.is_ref:
            L = ctypes.CDLL(DICTREF)
            L.refdict_load.restype = VP
            L.refdict_load.argtypes = [ctypes.c_char_p]
            L.refdict_free.argtypes = [VP]
            self._info, self._id, self._free = L.refdict_get_info, L.refdict_get_info_id, L.refdict_free
            self.h = L.refdict_load(path)
        else:
            L = ctypes.CDLL(bfutil.ORACLE_LIB)
            L.bfo_load_model.restype = VP
            L.bfo_load_model.argtypes = [ctypes.c_char_p]
            L.bfo_free_model.argtypes = [VP]
            self._info, self._id, self._free = L.bfo_dict_get_info, L.bfo_dict_get_info_id, L.bfo_free_model
            self.h = L.bfo_load_model(path)
        self._info.argtypes = [VP, VP, CI, VP, CI]
        self._id.argtypes = [VP, VP, CI]
        self._L = L
        assert self.h, model

    def lookup(self, key):
        """(ret, info id, values) of one key (a list of int symbols, none negative: FADictInterpreter_t.h:369-390 indexes its
        character map with the symbol, and the reference reads out of bounds on a negative one)"""
        arr = (ctypes.c_int32 * max(len(key), 1))(*key)
        out = (ctypes.c_int32 * self.MAX_OUT)()
        r = self._info(VP(self.h), arr, len(key), out, self.MAX_OUT)
        assert r <= self.MAX_OUT
        return r, self._id(VP(self.h), arr, len(key)), list(out[:max(r, 0)])

    def batch(self, keys):
        """-> (ret int32[n], ids int32[n], vals int32[total], val_off int64[n + 1])"""
        res = [self.lookup(k) for k in keys]
        ret = np.array([r for r, _, _ in res], dtype=np.int32)
        ids = np.array([i for _, i, _ in res], dtype=np.int32)
        vals, off = pack([np.array(v, dtype=np.int32) for _, _, v in res], np.int32)
        return ret, ids, vals, off

    def close(self):
        self._free(VP(self.h))


# ------------------------------------------------------------------------------------------------
# packing, tiling, digests
# ------------------------------------------------------------------------------------------------
def pack(items, dtype=np.uint8):
    """list of bytes / arrays -> (flat array, int64 offsets[n + 1])"""
    arrs = [np.frombuffer(x, dtype=np.uint8) if isinstance(x, (bytes, bytearray)) else np.asarray(x, dtype=dtype) for x in items]
    off = np.zeros(len(arrs) + 1, dtype=np.int64)
    if arrs:
        np.cumsum([len(a) for a in arrs], out=off[1:])
    flat = np.concatenate(arrs).astype(dtype, copy=False) if arrs else np.zeros(0, dtype=dtype)
    return np.ascontiguousarray(flat), off


def tile(flat, off, idx):
    """the batch whose item i is item idx[i] of (flat, off): no Python loop over the items"""
    idx = np.asarray(idx, dtype=np.int64)
    lens = (off[1:] - off[:-1])[idx]
    out_off = np.zeros(len(idx) + 1, dtype=np.int64)
    np.cumsum(lens, out=out_off[1:])
    src = np.repeat(off[:-1][idx] - out_off[:-1], lens) + np.arange(out_off[-1], dtype=np.int64)
    return np.ascontiguousarray(flat[src]), out_off


def tiling(nbase, n, seed):
    """n item numbers out of nbase: a seeded permutation repeated (the callers keep nbase odd, so the period is no multiple of 64
    or of the number of waves), every item used"""
    assert nbase % 2 == 1
    perm = np.random.RandomState(seed).permutation(nbase)
    return perm[np.arange(n, dtype=np.int64) % nbase]


def digest(x):
    """[length, sha256] of bytes or of an array: what tests/golden/ref_answers keeps of a large output"""
    raw = x if isinstance(x, (bytes, bytearray)) else np.ascontiguousarray(x).tobytes()
    return [len(x), hashlib.sha256(raw).hexdigest()]


def first_difference(g_off, w_off, items, what, names=None):
    """message naming the first item whose output size differs: index, name, input length, first bytes, both sizes"""
    if len(g_off) != len(w_off):
        return "%s: %d offsets, %d expected" % (what, len(g_off), len(w_off))
    bad = np.nonzero(np.diff(g_off) != np.diff(w_off))[0]
    if not len(bad):
        return "%s: offsets start at %d" % (what, g_off[0])
    d = int(bad[0])
    return "%s: %s: output size %d, expected %d" % (what, describe(items, d, names), g_off[d + 1] - g_off[d], w_off[d + 1] - w_off[d])


def describe(items, d, names=None):
    flat, off = items
    src = flat[off[d]:off[d + 1]]
    return "item %d of %d%s (input length %d, starts %r)" % (d, len(off) - 1, " '%s'" % names[d] if names else "", len(src),
                                                             src[:48].tobytes() if src.dtype == np.uint8 else src[:16].tolist())


# ------------------------------------------------------------------------------------------------
# NormalizeSpaces: features at the last bytes of a 64-byte window and the first of the next, with and without a byte order mark
# ------------------------------------------------------------------------------------------------
_FILL = b"abcdefghi jklmnopqrstuvwx yz0123456789ABCDE FGHIJ"


def _filler(n, shift=0):
    reps = (n + shift) // len(_FILL) + 2
    return (_FILL * reps)[shift:shift + n]


def _ws_run(n, kind):
    """n white-space characters: 0 = spaces, 1 = U+3000 (three bytes each), 2 = a mixture of one-, two- and three-byte ones"""
    if kind == 0:
        return b" " * n
    if kind == 1:
        return "　".encode() * n
    mix = [" ", "\t", " ", "　", "\n", " ", "﻿"]
    return "".join(mix[i % len(mix)] for i in range(n)).encode()


def _normsp_features():
    f = ["é", "好", "\U0001F600", "éé好好\U0001F600\U0001F600", "　", "▁", "x　y", "x▁y", "▁ ", " ▁", "▁   ▁",
         "_ ", " _", "_\t_", "\U0001F600 ", " \U0001F600", "　▁", "▁　", "q 　 r", "é é", "好　好"]
    f = [x.encode() for x in f]
    for n in (1, 63, 64, 65, 200):
        for kind in (0, 1, 2):
            f.append(b"L" + _ws_run(n, kind) + b"R")
    return f


def _place_features(min_bytes, shift):
    """every feature starting at the window offsets 60..66 (offsets count from the first byte after a byte order mark)"""
    buf = bytearray()
    feats = _normsp_features()
    rnd = 0
    while len(buf) < min_bytes:
        for k, f in enumerate(feats):
            for o in range(60, 67):
                pad = (o - len(buf)) % 64
                if pad < 5:
                    pad += 64
                buf += _filler(pad, (shift + k + o + rnd) % 40)
                assert len(buf) % 64 == o % 64
                buf += f
        rnd += 7
    return bytes(buf)


def normsp_docs():
    """[(name, bytes)]: see the module docstring of tests/test_secondary_edges.py"""
    body = _place_features(64 << 10, 0)
    docs = [("features_64k", body)]
    big = _place_features(1 << 20, 3)[:1 << 20]          # the 1 MiB cut may fall inside a character: end it at a character boundary
    while big and (big[-1] & 0xC0) == 0x80:
        big = big[:-1]
    if big and big[-1] >= 0xC0:
        big = big[:-1]
    docs.append(("features_1m", big))
    base = _filler(64 << 10, 5)
    for n in (1, 63, 64, 65, 200):
        for kind in (0, 1, 2):
            run = _ws_run(n, kind)
            docs.append(("only_ws_%d_%d" % (n, kind), run))
            docs.append(("leading_ws_%d_%d" % (n, kind), run + base))
        for o in range(60, 67):
            kind = (n + o) % 3
            cut = 64 * 1024 - 64 + o
            docs.append(("trailing_ws_%d_at%d" % (n, o), base[:cut - 1] + b"Z" + _ws_run(n, kind)))
            docs.append(("trailing_usp_ws_%d_at%d" % (n, o), base[:cut - 4] + b"Z" + "▁".encode() + _ws_run(n, kind)))
    docs.append(("trailing_ws_after_usp_space", base[:4000] + b" _" + b" " * 130))
    solid = base.replace(b" ", b"-")                          # no white space: also a uSpace that cannot be encoded leaves these their text
    docs.append(("no_ws", solid[:64 * 1000 + 61] + "é好\U0001F600".encode()))
    docs.append(("no_ws_then_trailing_run", solid[:64 * 1000 + 62] + _ws_run(70, 2)))
    docs.append(("leading_run_then_no_ws", _ws_run(65, 1) + solid[:64 * 1000]))
    docs.append(("no_ws_one_inner_space", solid[:64 * 1000 + 63] + b" " + solid[:100]))
    docs.append(("ws_usp_ws", b" " * 70 + "▁".encode() + b" " * 70 + b"_" + b" " * 70))
    # invalid UTF-8: the document yields nothing (tokdll:646-648)
    docs.append(("lone_continuation_at_window_start", base[:64 * 900] + b"\x96" + base[:100]))
    docs.append(("lone_continuation_at_end", base[:64 * 900 + 61] + b"\x96"))
    docs.append(("truncated_lead_at_window_start", base[:64 * 900] + b"\xe2\x96" + base[:100]))
    docs.append(("truncated_lead_at_end", base[:64 * 900 + 62] + b"\xe2\x96"))
    docs.append(("lead_at_window_end_valid", base[:64 * 900 + 63] + "▁好\U0001F600".encode() + base[:10]))
    out = []
    for name, b in docs:
        out.append((name, b))
        out.append(("bom_" + name, BOM + b))
    return out


# ------------------------------------------------------------------------------------------------
# TextToHashes
# ------------------------------------------------------------------------------------------------
def _tok(n, salt):
    """n bytes, none of them a space, many of them >= 0x80 (the hash sign-extends its bytes, tokdll:684-692)"""
    a = (np.arange(n, dtype=np.int64) * 37 + salt * 11 + 1) % 255 + 1
    a[a == 0x20] = 0xE9
    return a.astype(np.uint8).tobytes()


def hash_docs():
    docs = [("empty", b""), ("one_byte", b"a"), ("lengths", b" ".join(_tok(n, n) for n in (1, 63, 64, 65, 5000, 1, 64))),
            ("long_first", _tok(5000, 1) + b" x"), ("long_last", b"x " + _tok(5000, 2)),
            ("tokens_65", b" ".join(_tok(1 + i % 9, i) for i in range(65))), ("tokens_64", b" ".join(_tok(1 + i % 9, i) for i in range(64))),
            ("tokens_100000", b" ".join(_tok(1 + i % 7, i) for i in range(100000))),
            ("run_2", b"ab  cd"), ("run_70", b"ab" + b" " * 70 + b"cd"), ("leading", b" ab cd"), ("trailing", b"ab cd "), ("both", b" ab  cd "),
            ("high_bytes", "é 好 \U0001F600 ▁x".encode() + b" \xff\x80 \xfe")]
    for n in (1, 2, 63, 64, 65, 200):
        docs.append(("spaces_%d" % n, b" " * n))
    docs.append(("run_70_at_edge", _tok(60, 3) + b" " * 70 + _tok(3, 4) + b" " * 2 + _tok(64, 5)))
    return docs


# ------------------------------------------------------------------------------------------------
# IdsToText
# ------------------------------------------------------------------------------------------------
def i2w_count(model):
    ora = bfutil.oracle()
    ora.lib.bfo_i2w_count.argtypes = [VP]
    h = ora.load(bfutil.model_path(model))
    n = ora.lib.bfo_i2w_count(VP(h))
    ora.free(h)
    return n


def i2w_specials(ck, h, ntok):
    """the special tokens of a model, found by asking the checker: `plain` (text without a leading space), `space` (exactly " "),
    `lead` (starts with " " and goes on), `empty`, `outside` (a known id that skip_special leaves out); None where the model has none"""
    plain = None
    for i in range(ntok):
        t = ck.ids_to_text(h, [i], 0)
        if t and t[:1] != b" " and ck.ids_to_text(h, [i, i], 0) == t + t and ck.ids_to_text(h, [i], 1) == t:
            plain, ptext = i, t
            break
    assert plain is not None
    sp = {"plain": plain, "space": None, "lead": None, "empty": None, "outside": None}
    for i in range(ntok):
        raw = ck.ids_to_text(h, [plain, i], 0)[len(ptext):]       # behind a written token nothing is taken off (tokdll:1724-1728)
        kept = ck.ids_to_text(h, [plain, i], 1)[len(ptext):]
        if kept != raw:
            if sp["outside"] is None and raw:
                sp["outside"] = i
            continue
        if raw == b"":
            key = "empty"
        elif raw == b" ":
            key = "space"
        elif raw[:1] == b" ":
            key = "lead"
        else:
            continue
        if sp[key] is None:
            sp[key] = i
        if all(v is not None for v in sp.values()):
            break
    return sp


def i2t_sequences(sp, ntok):
    """[(name, int32 ids)]: the first solid token (neither skipped, empty nor exactly " ") at chosen positions of the 64-id windows"""
    seqs = []
    quiet = [sp[k] for k in ("space", "empty") if sp[k] is not None]                        # vanish in front of the first solid token
    quiet_skip = quiet + ([sp["outside"]] if sp["outside"] is not None else []) + [-1]      # ... when skip_special is set (-1: below every range)
    tail = [(7919 * i + 13) % ntok for i in range(150)]
    for label, pre in (("quiet", quiet), ("skipped", quiet_skip)):
        if not pre:
            continue
        for pos in (0, 1, 63, 64, 65, 127, 128, 1000):
            head = [pre[i % len(pre)] for i in range(pos)]
            for kind in ("plain", "lead"):
                if sp[kind] is not None:
                    seqs.append(("%s_%s_at%d" % (label, kind, pos), head + [sp[kind]] + tail))
                    seqs.append(("%s_%s_at%d_alone" % (label, kind, pos), head + [sp[kind]]))
        seqs.append(("%s_never_solid" % label, [pre[i % len(pre)] for i in range(300)]))
        seqs.append(("%s_never_solid_64" % label, [pre[i % len(pre)] for i in range(64)]))
    seqs.append(("ids_100000", [(104729 * i + 7) % ntok for i in range(100000)]))
    seqs.append(("ids_100000_quiet_head", [(quiet_skip[i % len(quiet_skip)] if i < 70000 else (31 * i) % ntok) for i in range(100000)]))
    good_a, good_b = tail[:90], [(17 * i + 5) % ntok for i in range(200)]
    long_good = [(613 * i + 29) % ntok for i in range(3000)]
    for unk in (-1, ntok):
        for where, pos in (("first", 0), ("at64", 64), ("last", 2999)):
            bad = list(long_good)
            bad[pos] = unk
            seqs += [("good_before_%s_%d" % (where, unk), good_a), ("unknown_%s_%d" % (where, unk), bad), ("good_after_%s_%d" % (where, unk), good_b)]
    return [(name, np.array(ids, dtype=np.int32)) for name, ids in seqs]


# ------------------------------------------------------------------------------------------------
# DictGetInfo
# ------------------------------------------------------------------------------------------------
def dict_edge_keys(model, dck):
    """keys of 0, 1, 299, 300, 301 symbols, proper prefixes of entries, then hits and misses in turn (the value offsets get gaps)"""
    import test_dict_lookup
    pool = test_dict_lookup.keys_for(model, n_random=1500, seed=7, negative=False)
    res = [dck.lookup(k) for k in pool]
    hits = [k for k, r in zip(pool, res) if r[0] > 0]
    miss = [k for k, r in zip(pool, res) if r[0] <= 0]
    assert len(hits) > 100 and len(miss) > 100, (model, len(hits), len(miss))
    keys = [[], [97], [97] * 299, [97] * 300, [97] * 301, [0x2581] + [97] * 299, [0x2581] + [97] * 300]
    longest = sorted(hits, key=len)[-40:]
    keys += [k[:-1] for k in longest if len(k) > 1] + [k[:1] for k in longest] + [k + [97] for k in longest] + longest
    n = min(len(hits), len(miss), 1200)
    for i in range(n):
        keys.append(hits[i])
        keys.append(miss[i])
        if i % 3 == 0:
            keys.append(miss[(i * 7) % len(miss)])
        if i % 5 == 0:
            keys.append(hits[(i * 11) % len(hits)])
    return keys


# ------------------------------------------------------------------------------------------------
# the mixed documents of the many-document batches
# ------------------------------------------------------------------------------------------------
def mixed_docs(nbase=2503):
    """documents whose neighbours differ: empty, one byte, invalid UTF-8, white space only, short lines, long ones"""
    fixed = [b"", b"a", b" ", b"\xff", b"\x80", BOM, b"\xe2\x96", b"ab  cd ", b" . ", "好".encode(), b"Hello world. This is a test! Is it?",
             "x　▁ y".encode(), b"\t\n", b"a b", b"", b"z"]
    fuzz = bfutil.fuzz_docs(nbase, seed=131)
    lines = bfutil.fuzz_docs(600, seed=137, maxwords=400)
    docs = []
    i = 0
    while len(docs) < nbase:
        docs.append(fixed[i % len(fixed)])
        docs.append(fuzz[i])
        if i % 9 == 0:
            docs.append(lines[(i // 9) % len(lines)])
        i += 1
    return docs[:nbase]


def short_docs(nbase=2503):
    """at most 24 bytes each: the batches of 300,000 documents are built from these"""
    docs = [d[:24] for d in mixed_docs(nbase)]
    return [d if i % 4 else d[:i % 7] for i, d in enumerate(docs)]


def i2t_mixed(ntok, nbase=2503, short=False, seed=9):
    import random
    rng = random.Random(seed)
    seqs = []
    for t in range(nbase):
        n = rng.choice([0, 1, 2, 3, 5] if short else [0, 1, 2, 5, 20, 100, 700, 64, 65])
        ids = [rng.randrange(0, ntok) for _ in range(n)]
        if t % 7 == 0 and n:
            ids[rng.randrange(n)] = rng.choice([-1, ntok, ntok + 5, 0, 1, 2, 3])
        if t % 11 == 0 and n > 2 and ntok > 50000:
            ids[0] = ids[1] = 220                        # gpt2 / roberta: id 220 is " " -- the leading-space rule
        seqs.append(np.array(ids, dtype=np.int32))
    return seqs
