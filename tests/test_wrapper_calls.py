"""CPU: what blingfire_amd/__init__.py sends to the C library, call by call, against a recording stand-in for the library.

No built library, model file or device is needed: the stand-in checks every call against the bound signature (arity, and
`from_param` of every argument), logs it as (symbol, arguments) with a pointer written as None (NULL) or "ptr", and answers what a
per-symbol script says; a script may write through a pointer argument, which is how the size answers of the capacity-retry and the
count-then-fill forms get back to the wrapper.  The Device forms run on CPU tensors (data_ptr() works there) with stream=9, or
with torch.cuda.current_stream / synchronize replaced by recorders.  A synchronisation shows in the log as ("<sync>", ()).

The second half checks the signature table itself against the two headers that declare the symbols.
"""
import ctypes
import os
import re
import types

import numpy as np
import pytest

import bfutil

P, N = "ptr", None
ERR = b"boom"


def _addr(a):
    if a is None:
        return 0
    if isinstance(a, bool):
        raise TypeError("a bool where an address belongs")
    if isinstance(a, int):
        return a
    if isinstance(a, ctypes.c_void_p):
        return a.value or 0
    if isinstance(a, bytes):
        return -1
    if hasattr(a, "_obj"):
        return ctypes.addressof(a._obj)
    return ctypes.addressof(a)


def _is_pointer(t):
    return t in (ctypes.c_void_p, ctypes.c_char_p) or issubclass(t, ctypes._Pointer)


def put64(a, i, v):
    ctypes.c_int64.from_address(_addr(a) + 8 * i).value = v


def put32(a, vals):
    for i, v in enumerate(vals):
        ctypes.c_int32.from_address(_addr(a) + 4 * i).value = v


def putbytes(a, b):
    ctypes.memmove(_addr(a), b, len(b))


class _Fn:
    def __init__(self, owner, name):
        self.owner, self.name, self.restype, self.argtypes = owner, name, ctypes.c_int, None

    def __call__(self, *args):
        argtypes = self.argtypes or []
        assert len(args) == len(argtypes), "%s: %d arguments for %d argtypes" % (self.name, len(args), len(argtypes))
        norm = []
        for t, a in zip(argtypes, args):
            t.from_param(a)
            if _is_pointer(t):
                norm.append(P if _addr(a) else N)
            else:
                norm.append(a.value if isinstance(a, ctypes._SimpleCData) else a)
        self.owner.log.append((self.name, tuple(norm)))
        self.owner.raw.append((self.name, args))
        s = self.owner.script.get(self.name, 0)
        if isinstance(s, list):
            s = s.pop(0)
        return s(*args) if callable(s) else s


class StandIn:
    """the library's place: attribute -> recording callable"""

    def __init__(self):
        self.__dict__.update(log=[], raw=[], script={"BfLastError": ERR}, fns={})

    def __getattr__(self, name):
        if name.startswith("_"):
            raise AttributeError(name)
        if name not in self.fns:
            self.fns[name] = _Fn(self, name)
        return self.fns[name]


@pytest.fixture
def env(monkeypatch):
    import torch
    import blingfire_amd as bf
    L = StandIn()
    monkeypatch.setattr(bf, "_lib", bf._bind(L))
    streams = []

    def current_stream(dev=None):
        streams.append(dev)
        return types.SimpleNamespace(cuda_stream=5)
    monkeypatch.setattr(torch.cuda, "current_stream", current_stream)
    monkeypatch.setattr(torch.cuda, "synchronize", lambda dev=None: L.log.append(("<sync>", ())))
    return types.SimpleNamespace(bf=bf, L=L, torch=torch, streams=streams)


def shapes(out):
    return [(tuple(x.shape), str(x.dtype).replace("torch.", "")) for x in out]


def raises(exc, text, fn, *a, **kw):
    with pytest.raises(exc) as e:
        fn(*a, **kw)
    assert str(e.value) == text


IDS, OFF = [1, 2, 3], [0, 2, 3]


def dev_ragged(torch):
    return torch.tensor(IDS, dtype=torch.int32), torch.tensor(OFF, dtype=torch.int64)


def dev_docs(torch):
    return torch.tensor([97, 98, 99], dtype=torch.uint8), torch.tensor(OFF, dtype=torch.int64)


# ------------------------------------------------------------------------------------------------
# loading, the reference-mirror single calls
# ------------------------------------------------------------------------------------------------
def test_lib_missing_raises(monkeypatch, tmp_path):
    import blingfire_amd as bf
    monkeypatch.setattr(bf, "_lib", None)
    monkeypatch.setattr(bf, "LIB_PATH", str(tmp_path / "none.so"))
    raises(RuntimeError, "%s is missing: run `python -m blingfire_amd.build` (hipcc, gfx950) first; there is no CPU fallback" % (tmp_path / "none.so"), bf.lib)


def test_version_load_free(env):
    bf, L = env.bf, env.L
    L.script.update(GetBlingFireTokVersion=18000, LoadModel=[7, None])
    assert bf.get_blingfiretok_version() == 18000
    assert bf.load_model("m.bin") == 7
    raises(RuntimeError, "LoadModel('m.bin') failed: boom", bf.load_model, "m.bin")
    bf.free_model(7)
    bf.change_settings_dummy_prefix(7, True)
    assert L.log == [("GetBlingFireTokVersion", ()), ("LoadModel", (P,)), ("LoadModel", (P,)), ("BfLastError", ()), ("FreeModel", (P,)),
                     ("SetNoDummyPrefix", (P, False))]
    assert L.raw[1][1] == (b"m.bin",)


def test_text_to_ids_single(env):
    bf, L = env.bf, env.L

    def answer(h, s, n, o, *rest):
        put32(o, [5, 6])
        return 2
    L.script.update(TextToIds=answer, TextToIdsWithOffsets=2)
    a = bf.text_to_ids(7, "ab", 4, unk=9)
    assert a.dtype == np.uint32 and a.tolist() == [5, 6, 0, 0]
    assert bf.text_to_ids(7, b"ab", 4, 9, no_padding=True).tolist() == [5, 6]
    assert shapes(bf.utf8text_to_ids_with_offsets(7, b"ab", 4, 9)) == [((4,), "uint32"), ((4,), "int32"), ((4,), "int32")]
    assert shapes(bf.utf8text_to_ids_with_offsets(7, b"ab", 4, 9, no_padding=True)) == [((2,), "uint32"), ((2,), "int32"), ((2,), "int32")]
    assert L.log == [("TextToIds", (P, P, 2, P, 4, 9))] * 2 + [("TextToIdsWithOffsets", (P, P, 2, P, P, P, 4, 9))] * 2


def test_single_string_calls(env):
    bf, L = env.bf, env.L

    def writes(text, at):
        def f(*args):
            putbytes(args[at], text + b"\0")
            return len(text)
        return f
    L.script.update(NormalizeSpaces=[writes(b"a b", 2), -1], WordHyphenationWithModel=[writes(b"a-b", 2), 100], TextToWords=[writes(b"a b", 2), -1],
                    TextToWordsWithModel=[writes(b"a b", 2), 7], TextToSentences=[writes(b"a b", 2), -1], TextToSentencesWithModel=[writes(b"a b", 2), 7])
    assert bf.normalize_spaces("a  b") == "a b" and bf.normalize_spaces("a  b", 0x5F) == ""
    assert bf.word_hyphenation_with_model(7, "ab") == "a-b" and bf.word_hyphenation_with_model(0, "ab", 0x2E) == ""     # (100 > the 9 byte buffer)
    assert bf.text_to_words("a b") == "a b" and bf.text_to_words("a b") == ""
    assert bf.text_to_words_with_model(7, "a b") == "a b" and bf.text_to_words_with_model(7, "ab") == ""              # (7 > the 6 byte buffer)
    assert bf.text_to_sentences("a b") == "a b" and bf.text_to_sentences("a b") == ""
    assert bf.text_to_sentences_with_model(7, "a b") == "a b" and bf.text_to_sentences_with_model(7, "a b") == ""     # (7 > the 6 byte buffer)
    assert L.log == [("NormalizeSpaces", (P, 4, P, 12, 0x20)), ("NormalizeSpaces", (P, 4, P, 12, 0x5F)),
                     ("WordHyphenationWithModel", (P, 2, P, 9, P, 0x2D)), ("WordHyphenationWithModel", (P, 2, P, 9, N, 0x2E)),
                     ("TextToWords", (P, 3, P, 9)), ("TextToWords", (P, 3, P, 9)),
                     ("TextToWordsWithModel", (P, 3, P, 9, P)), ("TextToWordsWithModel", (P, 2, P, 6, P)),
                     ("TextToSentences", (P, 3, P, 6)), ("TextToSentences", (P, 3, P, 6)),
                     ("TextToSentencesWithModel", (P, 3, P, 6, P)), ("TextToSentencesWithModel", (P, 3, P, 6, P))]


def test_text_to_hashes_and_ids_to_text(env):
    bf, L = env.bf, env.L

    def text(h, ids, n, o, cap, skip):
        putbytes(o, b"hi\0")
        return 2
    L.script.update(TextToHashes=[2, -1, 7], IdsToText=[text, -1, 9])
    got = bf.text_to_hashes("a b", 2, 100)
    assert got.dtype == np.int32 and got.shape == (2,)
    assert bf.text_to_hashes("a b", 2, 100) == "" and bf.text_to_hashes("a b", 2, 100) == ""        # (-1, and 7 > the capacity of 6)
    assert bf.ids_to_text(7, np.array([1, 2], dtype=np.uint32)) == "hi"
    assert bf.ids_to_text(7, [1, 2], False) == "" and bf.ids_to_text(7, [1, 2], output_buffer_size=8) == ""
    assert L.log == [("TextToHashes", (P, 3, P, 6, 2, 100))] * 3 + [("IdsToText", (P, P, 2, P, 64, True)), ("IdsToText", (P, P, 2, P, 64, False)),
                                                                   ("IdsToText", (P, P, 2, P, 8, True))]


def test_offsets_are_characters(env):
    bf, L = env.bf, env.L
    s = "é b"                                           # 4 bytes, 3 characters

    def words(sb, n, o, st, en, cap, h):
        putbytes(o, s.encode("utf-8") + b"\0"); put32(st, [0, 3]); put32(en, [1, 3])
        return 4

    def sents(sb, n, o, st, en, cap, h):
        putbytes(o, b"\xc3\xa9\nb\0"); put32(st, [0, 3]); put32(en, [1, 3])
        return 4
    L.script.update(TextToWordsWithOffsetsWithModel=[words, -1, 13], TextToSentencesWithOffsetsWithModel=[sents, -1, 9])
    assert bf.text_to_words_with_offsets(s) == (s, [(0, 1), (2, 3)])
    assert bf.text_to_words_with_offsets(s, 7) == ("", []) and bf.text_to_words_with_offsets(s) == ("", [])
    assert bf.text_to_sentences_and_offsets(s) == ("é\nb", [(0, 1), (2, 3)])
    assert bf.text_to_sentences_and_offsets(s, 7) == ("", []) and bf.text_to_sentences_and_offsets(s) == ("", [])
    assert L.log == [("TextToWordsWithOffsetsWithModel", (P, 4, P, P, P, 12, N)), ("TextToWordsWithOffsetsWithModel", (P, 4, P, P, P, 12, P)),
                     ("TextToWordsWithOffsetsWithModel", (P, 4, P, P, P, 12, N)),
                     ("TextToSentencesWithOffsetsWithModel", (P, 4, P, P, P, 8, N)), ("TextToSentencesWithOffsetsWithModel", (P, 4, P, P, P, 8, P)),
                     ("TextToSentencesWithOffsetsWithModel", (P, 4, P, P, P, 8, N))]


# ------------------------------------------------------------------------------------------------
# capacity retry: size call, -3, allocate from offsets[-1], call again
# ------------------------------------------------------------------------------------------------
def sized(at_out, at_off, n, total, fill=None):
    """a script for a capacity-retry symbol of n items: without an output it writes `total` into offsets[n] and answers -3"""
    def f(*args):
        put64(args[at_off], n, total)
        if _addr(args[at_out]) == 0 and total > 0:
            return -3
        if fill:
            putbytes(args[at_out], fill)
        return n
    return f


def test_word_hyphenation_batch(env):
    bf, L = env.bf, env.L

    def f(h, text, off, nw, out, cap, t_off, uhy):
        for i, v in enumerate([0, 3, 4]):
            put64(t_off, i, v)
        if out is None:
            return -3
        putbytes(out, b"a-bc")
        return 2
    L.script.update(WordHyphenationBatch=[f, f, 0, -2])
    assert bf.word_hyphenation_batch(7, ["ab", b"c"]) == ["a-b", "c"]
    assert bf.word_hyphenation_batch(7, [], 0x2E) == []
    raises(RuntimeError, "WordHyphenationBatch failed: -2 (boom)", bf.word_hyphenation_batch, 7, ["ab"])
    assert L.log == [("WordHyphenationBatch", (P, P, P, 2, N, 0, P, 0x2D)), ("WordHyphenationBatch", (P, P, P, 2, P, 4, P, 0x2D)),
                     ("WordHyphenationBatch", (P, P, P, 0, N, 0, P, 0x2E)), ("WordHyphenationBatch", (P, P, P, 1, N, 0, P, 0x2D)), ("BfLastError", ())]


@pytest.mark.parametrize("fn, sym", [("text_to_words_batch", "TextToWordsBatch"), ("text_to_sentences_batch", "TextToSentencesBatch")])
def test_text_to_words_batch(env, fn, sym):
    bf, L = env.bf, env.L
    L.script[sym] = [sized(4, 6, 2, 4), sized(4, 6, 2, 4, b"a bc"), sized(4, 6, 2, 0), -1]
    text, off = getattr(bf, fn)([b"ab", "c"])
    assert shapes([text, off]) == [((4,), "uint8"), ((3,), "int64")] and bytes(text) == b"a bc" and off[-1] == 4
    text, off = getattr(bf, fn)((np.frombuffer(b"abc", dtype=np.uint8), np.array(OFF)), 7)
    assert shapes([text, off]) == [((0,), "uint8"), ((3,), "int64")]
    raises(RuntimeError, "%s failed: -1 (boom)" % sym, getattr(bf, fn), [b"ab"])
    assert L.log == [(sym, (N, P, P, 2, N, 0, P)), (sym, (N, P, P, 2, P, 4, P)), (sym, (P, P, P, 2, N, 0, P)), (sym, (N, P, P, 1, N, 0, P)), ("BfLastError", ())]


def test_ids_to_text_batch(env):
    bf, L = env.bf, env.L
    L.script["IdsToTextBatch"] = [sized(4, 6, 2, 5), sized(4, 6, 2, 5, b"hello"), sized(4, 6, 2, 0), -2]
    text, off = bf.ids_to_text_batch(7, IDS, OFF)
    assert shapes([text, off]) == [((5,), "uint8"), ((3,), "int64")] and bytes(text) == b"hello"
    assert shapes(bf.ids_to_text_batch(7, IDS, OFF, skip_special_tokens=False)) == [((0,), "uint8"), ((3,), "int64")]
    raises(RuntimeError, "IdsToTextBatch failed: -2 (boom)", bf.ids_to_text_batch, 7, IDS, OFF)
    assert L.log == [("IdsToTextBatch", (P, P, P, 2, N, 0, P, 1)), ("IdsToTextBatch", (P, P, P, 2, P, 5, P, 1)), ("IdsToTextBatch", (P, P, P, 2, N, 0, P, 0)),
                     ("IdsToTextBatch", (P, P, P, 2, N, 0, P, 1)), ("BfLastError", ())]


def test_dict_get_info_batch(env):
    bf, L = env.bf, env.L

    def f(h, keys, off, nk, ret, ids, vals, cap, v_off):
        put32(ret, [2, 1]); put32(ids, [8, 9]); put64(v_off, 2, 3)            # the size pass fills the two per-key outputs
        if vals is None:
            return -3
        put32(vals, [4, 5, 6])
        return 2
    L.script["DictGetInfoBatch"] = [f, f, 0, -2]
    ret, ids, vals, v_off = bf.dict_get_info_batch(7, ["ab", [99]])
    assert shapes([ret, ids, vals, v_off]) == [((2,), "int32"), ((2,), "int32"), ((3,), "int32"), ((3,), "int64")]
    assert ret.tolist() == [2, 1] and ids.tolist() == [8, 9] and vals.tolist() == [4, 5, 6] and v_off[-1] == 3
    assert shapes(bf.dict_get_info_batch(7, (np.array(IDS), np.array(OFF)))) == [((2,), "int32"), ((2,), "int32"), ((0,), "int32"), ((3,), "int64")]
    raises(RuntimeError, "DictGetInfoBatch failed: -2 (boom)", bf.dict_get_info_batch, 7, [])
    assert L.log == [("DictGetInfoBatch", (P, P, P, 2, P, P, N, 0, P)), ("DictGetInfoBatch", (P, P, P, 2, P, P, P, 3, P)),
                     ("DictGetInfoBatch", (P, P, P, 2, P, P, N, 0, P)), ("DictGetInfoBatch", (P, P, P, 0, P, P, N, 0, P)), ("BfLastError", ())]


# ------------------------------------------------------------------------------------------------
# handle-level calls
# ------------------------------------------------------------------------------------------------
def test_handle_calls(env):
    bf, L = env.bf, env.L

    def grows(out):
        ctypes.c_longlong.from_address(_addr(out)).value = 3
        ctypes.c_longlong.from_address(_addr(out) + 8).value = 1
        return 0
    L.script.update(BfSetDevices=[0, -2], BfShardHandle=11, BfShardRanges=[0, -1], BfReserve=[0, -4], BfWorkspaceGrows=[grows, -1], BfLastKernelMs=[6, -1])
    bf.set_devices(7, [0, 1])
    raises(RuntimeError, "BfSetDevices failed (-2): boom", bf.set_devices, 7, [0])
    assert bf.shard_handle(7, 1) == 11
    assert shapes([bf.shard_ranges(OFF, 2)]) == [((3,), "int64")]
    raises(RuntimeError, "BfShardRanges failed (-1)", bf.shard_ranges, OFF, 2)
    bf.reserve(7, 10, 100, True)
    raises(RuntimeError, "BfReserve failed (-4): boom", bf.reserve, 7, 10, 100)
    assert bf.workspace_grows() == (3, 1)
    raises(RuntimeError, "BfWorkspaceGrows failed (-1)", bf.workspace_grows)
    assert bf.last_kernel_ms(7) == [0.0] * 6 and bf.last_kernel_ms(7) == []
    assert L.log == [("BfSetDevices", (P, P, 2)), ("BfSetDevices", (P, P, 1)), ("BfLastError", ()), ("BfShardHandle", (P, 1)), ("BfShardRanges", (P, 2, 2, P)),
                     ("BfShardRanges", (P, 2, 2, P)), ("BfReserve", (P, 10, 100, 1)), ("BfReserve", (P, 10, 100, 0)), ("BfLastError", ()),
                     ("BfWorkspaceGrows", (P,)), ("BfWorkspaceGrows", (P,)), ("BfLastKernelMs", (P, P, 6)), ("BfLastKernelMs", (P, P, 6))]


def test_pack_docs():
    import blingfire_amd as bf
    text, off = bf.pack_docs(["ab", b"c"])
    assert bytes(text) == b"abc" and off.tolist() == OFF and off.dtype == np.int64
    assert shapes(bf.pack_docs([])) == [((0,), "uint8"), ((1,), "int64")]


# ------------------------------------------------------------------------------------------------
# the tokenizer batch calls
# ------------------------------------------------------------------------------------------------
def test_text_to_ids_batch_host(env):
    bf, L = env.bf, env.L
    L.script.update(TextToIdsBatch=[3, 2, -2], TextToIdsWithOffsetsBatch=[3, -2])
    assert shapes(bf.text_to_ids_batch(7, [b"ab", "c"], 8, unk=5)) == [((3,), "int32"), ((3,), "int64")]
    assert shapes(bf.text_to_ids_batch(7, (np.frombuffer(b"abc", dtype=np.uint8), np.array(OFF)), 1)) == [((2,), "int32"), ((3,), "int64")]
    raises(RuntimeError, "TextToIdsBatch failed (-2): boom", bf.text_to_ids_batch, 7, [], 8)
    assert shapes(bf.text_to_ids_with_offsets_batch(7, [b"ab", "c"], 8, 5)) == [((3,), "int32")] * 3 + [((3,), "int64")]
    raises(RuntimeError, "TextToIdsWithOffsetsBatch failed (-2): boom", bf.text_to_ids_with_offsets_batch, 7, [b"ab"], -1)
    # the id capacity is min(2 * (bytes + ndocs), ndocs * max_len) + 1
    assert L.log == [("TextToIdsBatch", (P, P, P, 2, P, 11, P, 8, 5)), ("TextToIdsBatch", (P, P, P, 2, P, 3, P, 1, 0)), ("TextToIdsBatch", (P, P, P, 0, P, 1, P, 8, 0)),
                     ("BfLastError", ()), ("TextToIdsWithOffsetsBatch", (P, P, P, 2, P, P, P, 11, P, 8, 5)),
                     ("TextToIdsWithOffsetsBatch", (P, P, P, 1, P, P, P, 1, P, -1, 0)), ("BfLastError", ())]


def test_text_to_ids_batch_device(env):
    bf, L, torch = env.bf, env.L, env.torch
    d_text, d_off = dev_docs(torch)
    L.script.update(TextToIdsBatchDevice=[0, 0, 0, -2], TextToIdsWithOffsetsBatchDevice=[0, 0, -2], IdsToTextBatchDevice=[0, 0, -2])
    assert shapes(bf.text_to_ids_batch_device(7, d_text, d_off, 8, 5, stream=9)) == [((10,), "int32"), ((3,), "int64")]
    assert shapes(bf.text_to_ids_batch_device(7, d_text, d_off, 0)) == [((1,), "int32"), ((3,), "int64")]
    mine = torch.empty(6, dtype=torch.int32), torch.empty(3, dtype=torch.int64)
    got = bf.text_to_ids_batch_device(7, d_text, d_off, 8, out_ids=mine[0], out_off=mine[1], stream=9)
    assert got[0] is mine[0] and got[1] is mine[1]
    raises(RuntimeError, "TextToIdsBatchDevice failed (-2): boom", bf.text_to_ids_batch_device, 7, d_text, d_off, 8, stream=9)
    assert shapes(bf.text_to_ids_with_offsets_batch_device(7, d_text, d_off, 8, 5, stream=9)) == [((10,), "int32")] * 3 + [((3,), "int64")]
    assert shapes(bf.text_to_ids_with_offsets_batch_device(7, d_text, d_off, 0)) == [((1,), "int32")] * 3 + [((3,), "int64")]
    raises(RuntimeError, "TextToIdsWithOffsetsBatchDevice failed (-2): boom", bf.text_to_ids_with_offsets_batch_device, 7, d_text, d_off, 8, stream=9)
    d_ids = torch.tensor(IDS, dtype=torch.int32)
    assert shapes(bf.ids_to_text_batch_device(7, d_ids, d_off, stream=9)) == [((48,), "uint8"), ((3,), "int64")]
    got = bf.ids_to_text_batch_device(7, d_ids[:0], d_off, out_text=torch.empty(5, dtype=torch.uint8), skip_special_tokens=False)
    assert shapes(got) == [((5,), "uint8"), ((3,), "int64")]
    raises(RuntimeError, "IdsToTextBatchDevice failed (-2): boom", bf.ids_to_text_batch_device, 7, d_ids, d_off, stream=9)
    # the id capacity is max(1, min(2 * (bytes + ndocs), ndocs * max_len))
    assert L.log == [("TextToIdsBatchDevice", (P, P, P, 2, 3, P, 10, P, 8, 5, P)), ("TextToIdsBatchDevice", (P, P, P, 2, 3, P, 1, P, 0, 0, P)),
                     ("TextToIdsBatchDevice", (P, P, P, 2, 3, P, 6, P, 8, 0, P)), ("TextToIdsBatchDevice", (P, P, P, 2, 3, P, 10, P, 8, 0, P)), ("BfLastError", ()),
                     ("TextToIdsWithOffsetsBatchDevice", (P, P, P, 2, 3, P, P, P, 10, P, 8, 5, P)),
                     ("TextToIdsWithOffsetsBatchDevice", (P, P, P, 2, 3, P, P, P, 1, P, 0, 0, P)),
                     ("TextToIdsWithOffsetsBatchDevice", (P, P, P, 2, 3, P, P, P, 10, P, 8, 0, P)), ("BfLastError", ()),
                     ("IdsToTextBatchDevice", (P, P, P, 2, P, 48, P, 1, P)), ("IdsToTextBatchDevice", (P, N, P, 2, P, 5, P, 0, P)),     # (no ids: an empty tensor has no address)
                     ("IdsToTextBatchDevice", (P, P, P, 2, P, 48, P, 1, P)), ("BfLastError", ())]
    assert len(env.streams) == 3                                           # only the three calls without `stream` ask torch for one
    assert L.raw[0][1][-1].value == 9 and L.raw[1][1][-1].value == 5


# ------------------------------------------------------------------------------------------------
# the row stage: rows and pair rows
# ------------------------------------------------------------------------------------------------
ROWS_PRE = (P, P, P, 2, 4, 101, -1, 0, 0, 1, 0)
PAIR_PRE = (P, P, P, P, P, 2, 8, 101, 102, 0, 1, 0, 0, 1, 0)
ROWS5 = [((2, 4), "int32"), ((2, 4), "uint8"), ((2,), "int32"), ((2,), "int32"), ((3,), "int64")]
PAIR6 = [((2, 8), "int32"), ((2, 8), "uint8"), ((2, 8), "uint8"), ((2,), "int32"), ((2,), "int32"), ((3,), "int64")]


def test_ids_to_rows_batch(env):
    bf, L = env.bf, env.L
    L.script["IdsToRowsBatch"] = [2, 2, 0, -2, 2, 1]
    assert shapes(bf.ids_to_rows_batch(7, IDS, OFF, 4, cls_id=101)) == ROWS5
    got = bf.ids_to_rows_batch(7, IDS, OFF, 4, 101, 102, 9, 1, 0, True)                        # R = 0: no fill call
    assert shapes(got) == [((0, 4), "int32"), ((0, 4), "uint8"), ((0,), "int32"), ((0,), "int32"), ((3,), "int64")]
    raises(RuntimeError, "IdsToRowsBatch failed: -2 (boom)", bf.ids_to_rows_batch, 7, IDS, OFF, 4, cls_id=101)
    raises(RuntimeError, "IdsToRowsBatch failed: 1 (boom)", bf.ids_to_rows_batch, 7, IDS, OFF, 4, cls_id=101)
    query, fill = ("IdsToRowsBatch", ROWS_PRE + (N, N, N, N, 0, P)), ("IdsToRowsBatch", ROWS_PRE + (P, P, P, P, 2, P))
    assert L.log == [query, fill, ("IdsToRowsBatch", (P, P, P, 2, 4, 101, 102, 9, 1, 0, 1, N, N, N, N, 0, P)), query, ("BfLastError", ()), query, fill, ("BfLastError", ())]


def test_ids_to_rows_planes_batch(env):
    bf, L = env.bf, env.L
    L.script["IdsToRowsPlanesBatch"] = [2, 2, 0]
    *base, planes = bf.ids_to_rows_planes_batch(7, IDS, OFF, 4, cls_id=101, src=[[5, 6, 7]], fill=[-1])
    assert shapes(base) == ROWS5 and shapes(planes) == [((2, 4), "int32")]
    *base, planes = bf.ids_to_rows_planes_batch(7, IDS, OFF, 4, cls_id=101)
    assert len(base) == 5 and planes == []
    raises(ValueError, "companion planes: at most 4, and one source (or None) per fill value and side", bf.ids_to_rows_planes_batch, 7, IDS, OFF, 4, src=[IDS], fill=[])
    raises(ValueError, "companion planes: at most 4, and one source (or None) per fill value and side", bf.ids_to_rows_planes_batch, 7, IDS, OFF, 4, src=[None] * 5,
           fill=[0] * 5)
    assert L.log == [("IdsToRowsPlanesBatch", ROWS_PRE + (N, N, N, N, 0, P, 1, P, P, P)), ("IdsToRowsPlanesBatch", ROWS_PRE + (P, P, P, P, 2, P, 1, P, P, P)),
                     ("IdsToRowsPlanesBatch", ROWS_PRE + (N, N, N, N, 0, P, 0, P, P, P))]


def writes_total(at, i, total, ret=0):
    """a script for a Device size query: the total goes to element i of the int64 array at argument `at`"""
    def f(*args):
        put64(args[at], i, total)
        return ret
    return f


DROWS_PRE = (P, P, 3, P, 2, 4, 101, -1, 0, 0)


def test_ids_to_rows_batch_device(env):
    bf, L, torch = env.bf, env.L, env.torch
    d_ids, d_off = dev_ragged(torch)
    q = writes_total(17, 2, 2)
    L.script["IdsToRowsBatchDevice"] = [0, q, 0, q, 0, 0, -2]
    assert shapes(bf.ids_to_rows_batch_device(7, d_ids, d_off, 4, cls_id=101, stream=9)) == ROWS5          # one row per item is certain: no query
    assert shapes(bf.ids_to_rows_batch_device(7, d_ids, d_off, 4, cls_id=101, max_rows_per_seq=0, stream=9)) == ROWS5
    assert shapes(bf.ids_to_rows_batch_device(7, d_ids, d_off, 4, cls_id=101, max_rows_per_seq=0)) == ROWS5
    got = bf.ids_to_rows_batch_device(7, d_ids, d_off, 4, cls_id=101, max_rows_per_seq=0, rows_cap=5, stream=9)
    assert shapes(got) == [((5, 4), "int32"), ((5, 4), "uint8"), ((5,), "int32"), ((5,), "int32"), ((3,), "int64")]
    raises(RuntimeError, "IdsToRowsBatchDevice failed (-2): boom", bf.ids_to_rows_batch_device, 7, d_ids, d_off, 4, stream=9)
    one = ("IdsToRowsBatchDevice", DROWS_PRE + (1, 0, P, P, P, P, 2, P, P))
    query, fill = ("IdsToRowsBatchDevice", DROWS_PRE + (0, 0, N, N, N, N, 0, P, P)), ("IdsToRowsBatchDevice", DROWS_PRE + (0, 0, P, P, P, P, 2, P, P))
    assert L.log == [one, query, ("<sync>", ()), fill, query, fill, ("IdsToRowsBatchDevice", DROWS_PRE + (0, 0, P, P, P, P, 5, P, P)),
                     ("IdsToRowsBatchDevice", (P, P, 3, P, 2, 4, -1, -1, 0, 0, 1, 0, P, P, P, P, 2, P, P)), ("BfLastError", ())]
    assert len(env.streams) == 1


def test_ids_to_rows_planes_batch_device(env):
    bf, L, torch = env.bf, env.L, env.torch
    d_ids, d_off = dev_ragged(torch)
    L.script["IdsToRowsPlanesBatchDevice"] = [0, writes_total(17, 2, 2), 0]
    *base, planes = bf.ids_to_rows_planes_batch_device(7, d_ids, d_off, 4, cls_id=101, stream=9, src=[d_ids], fill=[-1])
    assert shapes(base) == ROWS5 and shapes(planes) == [((2, 4), "int32")]
    *base, planes = bf.ids_to_rows_planes_batch_device(7, d_ids, d_off, 4, cls_id=101, max_rows_per_seq=0, stream=9)
    assert shapes(base) == ROWS5 and planes == []
    raises(ValueError, "ids_to_rows_planes_batch_device: src[0] must be a contiguous torch.int32 tensor on cpu (got torch.int64, cpu, contiguous)",
           bf.ids_to_rows_planes_batch_device, 7, d_ids, d_off, 4, src=[d_off], fill=[0])
    raises(ValueError, "ids_to_rows_planes_batch_device: src[0] must be a contiguous torch.int32 tensor on cpu (got list)",
           bf.ids_to_rows_planes_batch_device, 7, d_ids, d_off, 4, src=[IDS], fill=[0])
    raises(ValueError, "ids_to_rows_planes_batch_device: src[0] must be a contiguous torch.int32 tensor on cpu (got torch.int32, cpu, not contiguous)",
           bf.ids_to_rows_planes_batch_device, 7, d_ids, d_off, 4, src=[torch.zeros((3, 2), dtype=torch.int32)[:, 0]], fill=[0])
    assert L.log == [("IdsToRowsPlanesBatchDevice", DROWS_PRE + (1, 0, P, P, P, P, 2, P, 1, P, P, P, P)),
                     ("IdsToRowsPlanesBatchDevice", DROWS_PRE + (0, 0, N, N, N, N, 0, P, 0, P, P, P, P)), ("<sync>", ()),
                     ("IdsToRowsPlanesBatchDevice", DROWS_PRE + (0, 0, P, P, P, P, 2, P, 0, P, P, P, P))]


def test_ids_to_pair_rows_batch(env):
    bf, L = env.bf, env.L
    A, B = (IDS, OFF), ([4, 5], [0, 1, 2])
    L.script.update(IdsToPairRowsBatch=[2, 2, 0, -2], IdsToPairRowsPlanesBatch=[2, 2, 0])
    assert shapes(bf.ids_to_pair_rows_batch(7, *A, *B, 8, cls_id=101, sep_id=102)) == PAIR6
    assert len(bf.ids_to_pair_rows_batch(7, *A, *B, 8, 101, 102, 9, 0, 2, 1, 0, True, True)) == 6
    raises(RuntimeError, "IdsToPairRowsBatch failed: -2 (boom)", bf.ids_to_pair_rows_batch, 7, *A, *B, 8)
    raises(ValueError, "ids_to_pair_rows_batch: off_a and off_b name different numbers of sequences", bf.ids_to_pair_rows_batch, 7, *A, [4, 5], [0, 2], 8)
    *base, planes = bf.ids_to_pair_rows_planes_batch(7, *A, *B, 8, cls_id=101, sep_id=102, src_b=[[8, 9]], fill=[-1])
    assert shapes(base) == PAIR6 and shapes(planes) == [((2, 8), "int32")]
    *base, planes = bf.ids_to_pair_rows_planes_batch(7, *A, *B, 8, cls_id=101, sep_id=102, src_a=[IDS, None], src_b=[None, [8, 9]], fill=[-1, -2])
    assert shapes(planes) == [((0, 8), "int32")] * 2
    raises(ValueError, "ids_to_pair_rows_planes_batch: off_a and off_b name different numbers of sequences", bf.ids_to_pair_rows_planes_batch, 7, *A, [4, 5], [0, 2], 8)
    raises(ValueError, "companion planes: at most 4, and one source (or None) per fill value and side", bf.ids_to_pair_rows_planes_batch, 7, *A, *B, 8, src_a=[IDS],
           fill=[0, 0])
    assert L.log == [("IdsToPairRowsBatch", PAIR_PRE + (N,) * 5 + (0, P)), ("IdsToPairRowsBatch", PAIR_PRE + (P,) * 5 + (2, P)),
                     ("IdsToPairRowsBatch", (P, P, P, P, P, 2, 8, 101, 102, 9, 0, 2, 1, 0, 3) + (N,) * 5 + (0, P)),
                     ("IdsToPairRowsBatch", (P, P, P, P, P, 2, 8, -1, -1, 0, 1, 0, 0, 1, 0) + (N,) * 5 + (0, P)), ("BfLastError", ()),
                     ("IdsToPairRowsPlanesBatch", PAIR_PRE + (N,) * 5 + (0, P, 1, P, P, P, P)), ("IdsToPairRowsPlanesBatch", PAIR_PRE + (P,) * 5 + (2, P, 1, P, P, P, P)),
                     ("IdsToPairRowsPlanesBatch", PAIR_PRE + (N,) * 5 + (0, P, 2, P, P, P, P))]


DPAIR_PRE = (P, P, 3, P, P, 2, P, 2, 8, 101, 102, 0)


def test_ids_to_pair_rows_batch_device(env):
    bf, L, torch = env.bf, env.L, env.torch
    a, a_off = dev_ragged(torch)
    b, b_off = torch.tensor([4, 5], dtype=torch.int32), torch.tensor([0, 1, 2], dtype=torch.int64)
    L.script.update(IdsToPairRowsBatchDevice=[0, 0, writes_total(23, 2, 2), 0, -2], IdsToPairRowsPlanesBatchDevice=[0, writes_total(23, 2, 2), 0])
    call = bf.ids_to_pair_rows_batch_device
    assert shapes(call(7, a, a_off, b, b_off, 8, cls_id=101, sep_id=102, stream=9)) == PAIR6                              # mode 1: one row per pair
    assert shapes(call(7, a, a_off, b, b_off, 8, cls_id=101, sep_id=102, mode=0, max_a=2, stride=1, stream=9)) == PAIR6    # max_rows_per_pair 1: the same
    assert shapes(call(7, a, a_off, b, b_off, 8, cls_id=101, sep_id=102, mode=0, max_rows_per_pair=0, double_sep=True, stream=9)) == PAIR6
    raises(RuntimeError, "IdsToPairRowsBatchDevice failed (-2): boom", call, 7, a, a_off, b, b_off, 8, cls_id=101, sep_id=102, rows_cap=3, stream=9)
    raises(ValueError, "ids_to_pair_rows_batch_device: d_off_a and d_off_b name different numbers of sequences", call, 7, a, a_off, b, b_off[:2], 8)
    call = bf.ids_to_pair_rows_planes_batch_device
    *base, planes = call(7, a, a_off, b, b_off, 8, cls_id=101, sep_id=102, stream=9, src_b=[b], fill=[-1])
    assert shapes(base) == PAIR6 and shapes(planes) == [((2, 8), "int32")]
    *base, planes = call(7, a, a_off, b, b_off, 8, cls_id=101, sep_id=102, mode=0, max_rows_per_pair=0)
    assert shapes(base) == PAIR6 and planes == []
    raises(ValueError, "ids_to_pair_rows_planes_batch_device: d_off_a and d_off_b name different numbers of sequences", call, 7, a, a_off, b, b_off[:2], 8)
    raises(ValueError, "ids_to_pair_rows_planes_batch_device: src_b[0] must be a contiguous torch.int32 tensor on cpu (got torch.int64, cpu, contiguous)",
           call, 7, a, a_off, b, b_off, 8, src_b=[b_off], fill=[0])
    outs, nulls = (P,) * 5, (N,) * 5
    assert L.log == [("IdsToPairRowsBatchDevice", DPAIR_PRE + (1, 0, 0, 1, 0) + outs + (2, P, P)),
                     ("IdsToPairRowsBatchDevice", DPAIR_PRE + (0, 2, 1, 1, 0) + outs + (2, P, P)),
                     ("IdsToPairRowsBatchDevice", DPAIR_PRE + (0, 0, 0, 0, 2) + nulls + (0, P, P)), ("<sync>", ()),
                     ("IdsToPairRowsBatchDevice", DPAIR_PRE + (0, 0, 0, 0, 2) + outs + (2, P, P)),
                     ("IdsToPairRowsBatchDevice", DPAIR_PRE + (1, 0, 0, 1, 0) + outs + (3, P, P)), ("BfLastError", ()),
                     ("IdsToPairRowsPlanesBatchDevice", DPAIR_PRE + (1, 0, 0, 1, 0) + outs + (2, P, 1, P, P, P, P, P)),
                     ("IdsToPairRowsPlanesBatchDevice", DPAIR_PRE + (0, 0, 0, 0, 0) + nulls + (0, P, 0, P, P, P, P, P)),
                     ("IdsToPairRowsPlanesBatchDevice", DPAIR_PRE + (0, 0, 0, 0, 0) + outs + (2, P, 0, P, P, P, P, P))]
    assert len(env.streams) == 1


def test_rows_span_cells_device(env):
    bf, L, torch = env.bf, env.L, env.torch
    st, en = torch.zeros((2, 4), dtype=torch.int32), torch.zeros((2, 4), dtype=torch.int32)
    seq, r_off = torch.zeros(2, dtype=torch.int32), torch.tensor([0, 1, 2], dtype=torch.int64)
    first, last = torch.tensor([0, 1]), torch.tensor([2, 3])
    L.script["RowsSpanCellsBatchDevice"] = [0, 0, -2]
    call = bf.rows_span_cells_device
    got = call(7, st, en, seq, r_off, first, last, none_cell=3, stream=9)
    assert shapes(got) == [((2,), "int32")] * 2 and got[0].tolist() == [3, 3] and got[1].tolist() == [3, 3]
    assert L.raw[0][1][5] == r_off.data_ptr() + 8 * 2                          # the address of the last row offset: the row count on the device
    assert shapes(call(7, st, en, None, None, first, last)) == [((2,), "int32")] * 2
    raises(RuntimeError, "RowsSpanCellsBatchDevice failed (-2): boom", call, 7, st, en, seq, r_off, first, last, stream=9)
    raises(ValueError, "rows_span_cells_device: starts must be a contiguous torch.int32 tensor on cpu (got torch.int64, cpu, contiguous)", call, 7, st.long(), en, seq,
           r_off, first, last)
    raises(ValueError, "rows_span_cells_device: row_seq must be a contiguous torch.int32 tensor on cpu (got list)", call, 7, st, en, [0, 0], r_off, first, last)
    raises(ValueError, "rows_span_cells_device: starts and ends are [R, L] planes of one shape, row_seq has R entries", call, 7, st, en[:1], seq, r_off, first, last)
    raises(ValueError, "rows_span_cells_device: starts and ends are [R, L] planes of one shape, row_seq has R entries", call, 7, st, en, seq[:1], r_off, first, last)
    raises(ValueError, "rows_span_cells_device: row_offsets must be a contiguous torch.int64 tensor on cpu", call, 7, st, en, seq, r_off.int(), first, last)
    raises(ValueError, "rows_span_cells_device: span_first / span_last need one entry per item (2)", call, 7, st, en, seq, r_off, first[:1], last[:1])
    raises(ValueError, "rows_span_cells_device: span_first / span_last need one entry per item (2)", call, 7, st, en, seq, None, first, last[:1])
    assert L.log == [("RowsSpanCellsBatchDevice", (P, P, P, 4, 2, P, P, 2, P, P, 3, P, P, P)), ("RowsSpanCellsBatchDevice", (P, P, P, 4, 2, N, N, 2, P, P, 0, P, P, P)),
                     ("RowsSpanCellsBatchDevice", (P, P, P, 4, 2, P, P, 2, P, P, 0, P, P, P)), ("BfLastError", ())]


# ------------------------------------------------------------------------------------------------
# packed rows and stream rows
# ------------------------------------------------------------------------------------------------
PACK_PRE = (P, P, P, 2, 4, 101, -1, 0, 0)
PACK6 = [((1, 4), "int32")] * 3 + [((2,), "int32")] * 3


def test_ids_to_packed_rows_batch(env):
    bf, L = env.bf, env.L
    L.script.update(IdsToPackedRowsBatch=[1, 1, 0, 0, -2, 1, 0], IdsToPackedRowsPlanesBatch=[1, 1])
    assert shapes(bf.ids_to_packed_rows_batch(7, IDS, OFF, 4, cls_id=101)) == PACK6
    got = bf.ids_to_packed_rows_batch(7, IDS, OFF, 4, 101, 102, 9)                              # R = 0: the fill call all the same (row_first_seq has R + 1 entries)
    assert shapes(got) == [((0, 4), "int32")] * 3 + [((1,), "int32"), ((2,), "int32"), ((2,), "int32")]
    raises(RuntimeError, "IdsToPackedRowsBatch failed: -2 (boom)", bf.ids_to_packed_rows_batch, 7, IDS, OFF, 4, cls_id=101)
    raises(RuntimeError, "IdsToPackedRowsBatch failed: 0 (boom)", bf.ids_to_packed_rows_batch, 7, IDS, OFF, 4, cls_id=101)
    *base, planes = bf.ids_to_packed_rows_planes_batch(7, IDS, OFF, 4, cls_id=101, src=[IDS], fill=[-1])
    assert shapes(base) == PACK6 and shapes(planes) == [((1, 4), "int32")]
    query, fill = ("IdsToPackedRowsBatch", PACK_PRE + (N, N, N, N, 0, P, P)), ("IdsToPackedRowsBatch", PACK_PRE + (P, P, P, P, 1, P, P))
    assert L.log == [query, fill, ("IdsToPackedRowsBatch", (P, P, P, 2, 4, 101, 102, 9, 0, N, N, N, N, 0, P, P)),
                     ("IdsToPackedRowsBatch", (P, P, P, 2, 4, 101, 102, 9, 0, P, P, P, P, 0, P, P)), query, ("BfLastError", ()), query, fill, ("BfLastError", ()),
                     ("IdsToPackedRowsPlanesBatch", PACK_PRE + (N, N, N, N, 0, P, P, 1, P, P, P)), ("IdsToPackedRowsPlanesBatch", PACK_PRE + (P, P, P, P, 1, P, P, 1, P, P, P))]


DPACK_PRE = (P, P, 3, P, 2, 4, 101, -1, 0, 0)
DPACK7 = PACK6 + [((1,), "int64")]


def test_ids_to_packed_rows_batch_device(env):
    bf, L, torch = env.bf, env.L, env.torch
    d_ids, d_off = dev_ragged(torch)
    q = writes_total(17, 0, 1)
    L.script.update(IdsToPackedRowsBatchDevice=[q, 0, q, 0, 0, -2], IdsToPackedRowsPlanesBatchDevice=[q, 0, 0])
    call = bf.ids_to_packed_rows_batch_device
    assert shapes(call(7, d_ids, d_off, 4, cls_id=101, stream=9)) == DPACK7
    assert shapes(call(7, d_ids, d_off, 4, cls_id=101)) == DPACK7
    got = call(7, d_ids, d_off, 4, cls_id=101, rows_cap=3, stream=9)
    assert shapes(got) == [((3, 4), "int32")] * 3 + [((4,), "int32"), ((2,), "int32"), ((2,), "int32"), ((1,), "int64")]
    raises(RuntimeError, "IdsToPackedRowsBatchDevice failed (-2): boom", call, 7, d_ids, d_off, 4, cls_id=101, stream=9)
    assert shapes(call(7, d_ids, d_off, 4, cls_id=101, stream=9, planes=[d_ids], fill=[-1])) == DPACK7 + [((1, 4), "int32")]
    assert shapes(call(7, d_ids, d_off, 4, cls_id=101, rows_cap=1, stream=9, planes=[])) == DPACK7          # an empty list is still the Planes symbol
    raises(ValueError, "ids_to_packed_rows_batch_device: fill without planes", call, 7, d_ids, d_off, 4, fill=[0])
    raises(ValueError, "ids_to_packed_rows_batch_device: planes[0] must be a contiguous torch.int32 tensor on cpu (got torch.int64, cpu, contiguous)", call, 7, d_ids,
           d_off, 4, planes=[d_off], fill=[0])
    raises(ValueError, "companion planes: at most 4, and one source (or None) per fill value and side", call, 7, d_ids, d_off, 4, planes=[d_ids])
    query = ("IdsToPackedRowsBatchDevice", DPACK_PRE + (N, N, N, N, 0, N, N, P, P))
    fill = ("IdsToPackedRowsBatchDevice", DPACK_PRE + (P, P, P, P, 1, P, P, P, P))
    assert L.log == [query, ("<sync>", ()), fill, query, fill, ("IdsToPackedRowsBatchDevice", DPACK_PRE + (P, P, P, P, 3, P, P, P, P)), query, ("BfLastError", ()),
                     ("IdsToPackedRowsPlanesBatchDevice", DPACK_PRE + (N, N, N, N, 0, N, N, P, 1, P, P, P, P)), ("<sync>", ()),
                     ("IdsToPackedRowsPlanesBatchDevice", DPACK_PRE + (P, P, P, P, 1, P, P, P, 1, P, P, P, P)),
                     ("IdsToPackedRowsPlanesBatchDevice", DPACK_PRE + (P, P, P, P, 1, P, P, P, 0, P, P, P, P))]
    assert len(env.streams) == 1


STREAM_PRE = (P, P, P, 2, 4, -1, 2, 0, -100, 0)


def test_ids_to_stream_rows_batch(env):
    bf, L = env.bf, env.L
    L.script["IdsToStreamRowsBatch"] = [2, 2, 0, 0, -2, 2, 1]
    got = bf.ids_to_stream_rows_batch(7, IDS, OFF, 4, eos_id=2)
    assert shapes(got) == [((2, 4), "int32")] * 4 + [((2,), "int32")] * 4
    got = bf.ids_to_stream_rows_batch(7, IDS, OFF, 4, 1, 2, 9, -1, True, True, True)             # R = 0: the second call all the same
    assert shapes(got) == [((0, 4), "int32")] * 4 + [((0,), "int32")] * 2 + [((2,), "int32")] * 2
    raises(RuntimeError, "IdsToStreamRowsBatch failed: -2 (boom)", bf.ids_to_stream_rows_batch, 7, IDS, OFF, 4, eos_id=2)
    raises(RuntimeError, "IdsToStreamRowsBatch failed: 1 (boom)", bf.ids_to_stream_rows_batch, 7, IDS, OFF, 4, eos_id=2)
    query, fill = ("IdsToStreamRowsBatch", STREAM_PRE + (N,) * 6 + (0, P, P)), ("IdsToStreamRowsBatch", STREAM_PRE + (P,) * 6 + (2, P, P))
    assert L.log == [query, fill, ("IdsToStreamRowsBatch", (P, P, P, 2, 4, 1, 2, 9, -1, 7) + (N,) * 6 + (0, P, P)),
                     ("IdsToStreamRowsBatch", (P, P, P, 2, 4, 1, 2, 9, -1, 7) + (P,) * 6 + (0, P, P)), query, ("BfLastError", ()), query, fill, ("BfLastError", ())]


def test_ids_to_stream_rows_batch_device(env):
    bf, L, torch = env.bf, env.L, env.torch
    d_ids, d_off = dev_ragged(torch)
    L.script["IdsToStreamRowsBatchDevice"] = [0, 0, 0, -2]
    call = bf.ids_to_stream_rows_batch_device
    got = call(7, d_ids, d_off, 4, eos_id=2, stream=9)                      # never a size query: the host bound ceil((3 + 1 * 2) / 4)
    assert shapes(got) == [((2, 4), "int32")] * 4 + [((2,), "int32")] * 4 + [((2,), "int64")]
    assert shapes(call(7, d_ids, d_off, 4, 1, 2, 9, -1, True, False, True))[:5] == [((2, 4), "int32")] * 4 + [((2,), "int32")]     # ceil((3 + 2 * 2) / 4)
    assert shapes(call(7, d_ids, d_off, 4, rows_cap=5, stream=9))[:5] == [((5, 4), "int32")] * 4 + [((5,), "int32")]
    raises(RuntimeError, "IdsToStreamRowsBatchDevice failed (-2): boom", call, 7, d_ids, d_off, 2, stream=9)
    assert L.log == [("IdsToStreamRowsBatchDevice", (P, P, 3, P, 2, 4, -1, 2, 0, -100, 0) + (P,) * 6 + (2, P, P, P, P)),
                     ("IdsToStreamRowsBatchDevice", (P, P, 3, P, 2, 4, 1, 2, 9, -1, 5) + (P,) * 6 + (2, P, P, P, P)),
                     ("IdsToStreamRowsBatchDevice", (P, P, 3, P, 2, 4, -1, -1, 0, -100, 0) + (P,) * 6 + (5, P, P, P, P)),
                     ("IdsToStreamRowsBatchDevice", (P, P, 3, P, 2, 2, -1, -1, 0, -100, 0) + (P,) * 6 + (2, P, P, P, P)), ("BfLastError", ())]
    assert len(env.streams) == 1


# ------------------------------------------------------------------------------------------------
# MLM masking and span corruption
# ------------------------------------------------------------------------------------------------
MLM_KW = dict(mask_id=103, rand_range=(5, 10), seed=-1, epoch=2 ** 32 + 3)
MLM20 = (P, P, 4, 2, N, N, N, N, N, 0, P, 0.15, 0.8, 0.1, 103, 5, 10, -100, 2 ** 64 - 1, 3)


def test_rows_mlm_mask_device(env):
    bf, L, torch = env.bf, env.L, env.torch
    rows = torch.arange(8, dtype=torch.int32).reshape(2, 4)
    mask, seg = torch.ones((2, 4), dtype=torch.uint8), torch.ones((2, 4), dtype=torch.int32)
    st, nrows = torch.zeros((2, 4), dtype=torch.int32), torch.tensor([2])
    L.script.update(RowsMlmMaskBatchDevice=[0, 0, -2], RowsMlmPredictionsBatchDevice=[0, -2])
    call = bf.rows_mlm_mask_device
    ids, labels = call(7, rows, stream=9, **MLM_KW)
    assert shapes([ids, labels]) == [((2, 4), "int32")] * 2 and ids is not rows and torch.equal(ids, rows) and labels.unique().tolist() == [-100]
    ids, labels = call(7, rows, mask=mask, seg=seg, starts=st, ends=st, nrows=nrows, special_ids=[1, 2, 3], select_prob=0.5, mask_prob=0.25, random_prob=0.125, mask_id=4,
                       rand_range=(6, 7), ignore_label=-1, seed=8, inplace=True)
    assert ids is rows and labels.unique().tolist() == [-1]
    assert list(ctypes.cast(L.raw[1][1][10], ctypes.POINTER(ctypes.c_int32))[0:3]) == [1, 2, 3]
    raises(RuntimeError, "RowsMlmMaskBatchDevice failed (-2): boom", call, 7, rows, stream=9, **MLM_KW)
    got = call(7, rows, stream=9, max_predictions=2, **MLM_KW)
    assert shapes(got) == [((2, 4), "int32")] * 2 + [((2, 2), "int32")] * 2 + [((2,), "int32")]
    assert [t.unique().tolist() for t in got[1:]] == [[-100], [0], [-100], [0]]
    raises(RuntimeError, "RowsMlmPredictionsBatchDevice failed (-2): boom", call, 7, rows, stream=9, max_predictions=np.int64(1), **MLM_KW)
    assert L.log == [("RowsMlmMaskBatchDevice", MLM20 + (P, P, P)),
                     ("RowsMlmMaskBatchDevice", (P, P, 4, 2, P, P, P, P, P, 3, P, 0.5, 0.25, 0.125, 4, 6, 7, -1, 8, 0, P, P, P)),
                     ("RowsMlmMaskBatchDevice", MLM20 + (P, P, P)), ("BfLastError", ()),
                     ("RowsMlmPredictionsBatchDevice", MLM20 + (P, P, 2, P, P, P, P)), ("RowsMlmPredictionsBatchDevice", MLM20 + (P, P, 1, P, P, P, P)), ("BfLastError", ())]
    assert len(env.streams) == 1
    del L.log[:]
    fn = "rows_mlm_mask_device: "
    raises(ValueError, fn + "rows must be a contiguous torch.int32 tensor on cpu (got torch.int64, cpu, contiguous)", call, 7, rows.long(), **MLM_KW)
    raises(ValueError, fn + "seg must be a contiguous torch.int32 tensor on cpu (got torch.uint8, cpu, contiguous)", call, 7, rows, seg=mask, **MLM_KW)
    raises(ValueError, fn + "ends must be a contiguous torch.int32 tensor on cpu (got list)", call, 7, rows, starts=st, ends=[1], **MLM_KW)
    raises(ValueError, fn + "rows is an [R, L] plane; mask, seg, starts and ends have its shape", call, 7, rows[0], **MLM_KW)
    raises(ValueError, fn + "rows is an [R, L] plane; mask, seg, starts and ends have its shape", call, 7, rows, mask=mask[:1], **MLM_KW)
    raises(ValueError, fn + "mask must be a contiguous torch.uint8 tensor on cpu", call, 7, rows, mask=seg, **MLM_KW)
    raises(ValueError, fn + "starts and ends come together", call, 7, rows, starts=st, **MLM_KW)
    raises(ValueError, fn + "nrows must be a torch.int64 tensor of one element on cpu", call, 7, rows, nrows=torch.tensor([2, 2]), **MLM_KW)
    raises(ValueError, fn + "nrows must be a torch.int64 tensor of one element on cpu", call, 7, rows, nrows=2, **MLM_KW)
    raises(ValueError, fn + "at most 8 special ids", call, 7, rows, special_ids=range(9), **MLM_KW)
    for bad in (-1, True, 1.0):
        raises(ValueError, fn + "max_predictions is an integer >= 0", call, 7, rows, max_predictions=bad, **MLM_KW)
    raises(ValueError, fn + "max_predictions needs rows of at most 4096 cells and is at most 1 << 20", call, 7, rows, max_predictions=(1 << 20) + 1, **MLM_KW)
    raises(ValueError, fn + "max_predictions needs rows of at most 4096 cells and is at most 1 << 20", call, 7, torch.zeros((1, 4097), dtype=torch.int32),
           max_predictions=1, **MLM_KW)
    assert L.log == []


DEN_KW = dict(start_prob=0.5, sentinel_first=32099, seed=-1, epoch=2 ** 32 + 3)


def test_rows_denoise_device(env):
    bf, L, torch = env.bf, env.L, env.torch
    rows = torch.arange(8, dtype=torch.int32).reshape(2, 4)
    mask, seg, nrows = torch.ones((2, 4), dtype=torch.uint8), torch.ones((2, 4), dtype=torch.int32), torch.tensor([2])
    L.script["RowsDenoiseBatchDevice"] = [0, 0, -2]
    call = bf.rows_denoise_device
    out = call(7, rows, stream=9, **DEN_KW)
    assert list(out) == ["input_ids", "labels", "enc_count", "dec_count", "span_count"]
    assert shapes(out.values()) == [((2, 4), "int32"), ((2, 6), "int32")] + [((2,), "int32")] * 3
    assert [t.unique().tolist() for t in out.values()] == [[0], [-100], [0], [0], [0]]
    out = call(7, rows, mask=mask, seg=seg, nrows=nrows, special_ids=[1, 2], start_prob=0.25, len_lo=2, len_hi=3, sentinel_first=50, sentinel_step=1, max_sentinels=9,
               eos_id=1, pad_id=7, ignore_label=-1, seed=8, enc_len=3, dec_len=5, return_cells=True)
    assert list(out) == ["input_ids", "labels", "enc_count", "dec_count", "span_count", "enc_cells", "dec_cells"]
    assert shapes(out.values()) == [((2, 3), "int32"), ((2, 5), "int32")] + [((2,), "int32")] * 3 + [((2, 3), "int32"), ((2, 5), "int32")]
    assert [t.unique().tolist() for t in out.values()] == [[7], [-1], [0], [0], [0], [-1], [-1]]
    raises(RuntimeError, "RowsDenoiseBatchDevice failed (-2): boom", call, 7, rows, stream=9, **DEN_KW)
    assert L.log == [("RowsDenoiseBatchDevice", (P, P, 4, 2, N, N, N, 0, P, 0.5, 1, 5, 32099, -1, 100, -1, 0, -100, 2 ** 64 - 1, 3, 4, P, N, P, 6, P, N, P, P, P)),
                     ("RowsDenoiseBatchDevice", (P, P, 4, 2, P, P, P, 2, P, 0.25, 2, 3, 50, 1, 9, 1, 7, -1, 8, 0, 3, P, P, P, 5, P, P, P, P, P)),
                     ("RowsDenoiseBatchDevice", (P, P, 4, 2, N, N, N, 0, P, 0.5, 1, 5, 32099, -1, 100, -1, 0, -100, 2 ** 64 - 1, 3, 4, P, N, P, 6, P, N, P, P, P)),
                     ("BfLastError", ())]
    assert len(env.streams) == 1
    del L.log[:]
    fn = "rows_denoise_device: "
    raises(ValueError, fn + "rows must be a contiguous torch.int32 tensor on cpu (got torch.int64, cpu, contiguous)", call, 7, rows.long(), **DEN_KW)
    raises(ValueError, fn + "seg must be a contiguous torch.int32 tensor on cpu (got torch.uint8, cpu, contiguous)", call, 7, rows, seg=mask, **DEN_KW)
    raises(ValueError, fn + "rows is an [R, L] plane; mask and seg have its shape", call, 7, rows[0], **DEN_KW)
    raises(ValueError, fn + "rows is an [R, L] plane; mask and seg have its shape", call, 7, rows, seg=seg[:1], **DEN_KW)
    raises(ValueError, fn + "mask must be a contiguous torch.uint8 tensor on cpu", call, 7, rows, mask=seg, **DEN_KW)
    raises(ValueError, fn + "nrows must be a torch.int64 tensor of one element on cpu", call, 7, rows, nrows=torch.tensor([2]).int(), **DEN_KW)
    raises(ValueError, fn + "at most 8 special ids", call, 7, rows, special_ids=range(9), **DEN_KW)
    raises(ValueError, fn + "enc_len and dec_len are at least 1", call, 7, rows, enc_len=0, **DEN_KW)
    raises(ValueError, fn + "enc_len and dec_len are at least 1", call, 7, rows, dec_len=0, **DEN_KW)
    assert L.log == []


def test_denoise_start_prob():
    import blingfire_amd as bf
    assert bf.denoise_start_prob(0.0) == 0.0 and bf.denoise_start_prob(1.0) == 1.0 and bf.denoise_start_prob(0.15, 1, 1) == pytest.approx(0.15, abs=1e-15)
    for bad in ((-0.1,), (1.5,), (0.5, 0, 5), (0.5, 3, 2)):
        raises(ValueError, "denoise_start_prob: noise_density in [0, 1] and 1 <= len_lo <= len_hi", bf.denoise_start_prob, *bad)


# ------------------------------------------------------------------------------------------------
# the encode_* chains: which calls, in which order (every one on torch's current stream)
# ------------------------------------------------------------------------------------------------
def names(L):
    return [n for n, _ in L.log]


def test_encode_batch_device(env):
    bf, L, torch = env.bf, env.L, env.torch
    d_text, d_off = dev_docs(torch)
    L.script.update(IdsToRowsBatchDevice=[0, writes_total(17, 2, 2), 0], IdsToRowsPlanesBatchDevice=[writes_total(17, 2, 2), 0])
    assert shapes(bf.encode_batch_device(7, d_text, d_off, 4, 101, 102, 0, unk=5)) == [ROWS5[0], ROWS5[1], ROWS5[2], ROWS5[4]]
    assert len(bf.encode_batch_device(7, d_text, d_off, 4, 101, None, 0, stride=1, max_rows_per_doc=0, pad_left=True)) == 4
    got = bf.encode_batch_device(7, d_text, d_off, 4, 101, 102, 0, max_rows_per_doc=2, return_offsets=True)
    assert shapes(got) == [ROWS5[0], ROWS5[1], ROWS5[2], ROWS5[4]] + [((2, 4), "int32")] * 2
    # max_len is what the rows can hold: body + (max_rows - 1) * (body - stride), all of it for max_rows 0
    assert L.log == [("TextToIdsBatchDevice", (P, P, P, 2, 3, P, 4, P, 2, 5, P)), ("IdsToRowsBatchDevice", (P, P, 4, P, 2, 4, 101, 102, 0, 0, 1, 0, P, P, P, P, 2, P, P)),
                     ("TextToIdsBatchDevice", (P, P, P, 2, 3, P, 10, P, 2 ** 31 - 1, 0, P)),
                     ("IdsToRowsBatchDevice", (P, P, 10, P, 2, 4, 101, -1, 0, 1, 0, 1, N, N, N, N, 0, P, P)),
                     ("IdsToRowsBatchDevice", (P, P, 10, P, 2, 4, 101, -1, 0, 1, 0, 1, P, P, P, P, 2, P, P)),
                     ("TextToIdsWithOffsetsBatchDevice", (P, P, P, 2, 3, P, P, P, 8, P, 4, 0, P)),
                     ("IdsToRowsPlanesBatchDevice", (P, P, 8, P, 2, 4, 101, 102, 0, 0, 2, 0, N, N, N, N, 0, P, 2, P, P, P, P)),
                     ("IdsToRowsPlanesBatchDevice", (P, P, 8, P, 2, 4, 101, 102, 0, 0, 2, 0, P, P, P, P, 2, P, 2, P, P, P, P))]
    for bad in (dict(L=2), dict(L=4, stride=-1), dict(L=4, stride=2), dict(L=4, max_rows_per_doc=-1)):
        kw = dict(L=bad.pop("L"), cls_id=101, sep_id=102, pad_id=0, **bad)
        raises(ValueError, "encode_batch_device: L leaves no room for ids, or stride / max_rows_per_doc are out of range", bf.encode_batch_device, 7, d_text, d_off, **kw)


def test_encode_pairs_and_qa_batch_device(env):
    bf, L, torch = env.bf, env.L, env.torch
    d_text, d_off = dev_docs(torch)
    q = writes_total(23, 2, 2)
    L.script.update(IdsToPairRowsBatchDevice=[0, q, 0], IdsToPairRowsPlanesBatchDevice=[0, 0, q, 0, q, 0])
    pairs, qa = bf.encode_pairs_batch_device, bf.encode_qa_batch_device
    assert shapes(pairs(7, d_text, d_off, d_text, d_off, 8, 101, 102, 0, unk=5)) == PAIR6
    assert shapes(pairs(7, d_text, d_off, d_text, d_off, 8, 101, 102, 0, mode=0, max_a=2, stride=1, max_rows_per_pair=2, double_sep=True)) == PAIR6
    assert names(L) == ["TextToIdsBatchDevice", "TextToIdsBatchDevice", "IdsToPairRowsBatchDevice"] * 2 + ["IdsToPairRowsBatchDevice"]      # (two rows a pair: a size query)
    # mode 1: both sides up to T = L - specials; mode 0: max_a for A and T + (max_rows - 1) * (T - stride) for B
    assert [a[8] for _, a in L.log if len(a) == 11] == [5, 5, 2, 4 + 3]
    assert L.log[5][1][8:17] == (8, 101, 102, 0, 0, 2, 1, 2, 2)
    del L.log[:]
    assert shapes(pairs(7, d_text, d_off, d_text, d_off, 8, 101, 102, 0, return_offsets=True)) == PAIR6 + [((2, 8), "int32")] * 2
    assert shapes(pairs(7, d_text, d_off, d_text, d_off, 8, 101, 102, 0, return_offsets=True, offsets_a=True)) == PAIR6 + [((2, 8), "int32")] * 2
    assert names(L) == ["TextToIdsBatchDevice", "TextToIdsWithOffsetsBatchDevice", "IdsToPairRowsPlanesBatchDevice",
                        "TextToIdsWithOffsetsBatchDevice", "TextToIdsWithOffsetsBatchDevice", "IdsToPairRowsPlanesBatchDevice"]
    assert L.log[2][1][23:] == (P, 2, P, P, P, P, P)
    del L.log[:]
    assert shapes(qa(7, d_text, d_off, d_text, d_off, 8, 101, 102, 0, 2, 1)) == PAIR6 + [((2, 8), "int32")] * 2
    first = torch.tensor([0, 1], dtype=torch.int32)
    got = qa(7, d_text, d_off, d_text, d_off, 8, 101, 102, 0, 2, 1, d_ans_first=first, d_ans_last=first)
    assert shapes(got) == PAIR6 + [((2, 8), "int32")] * 2 + [((2,), "int32")] * 2
    chain = ["TextToIdsBatchDevice", "TextToIdsWithOffsetsBatchDevice", "IdsToPairRowsPlanesBatchDevice", "IdsToPairRowsPlanesBatchDevice"]
    assert names(L) == chain + chain + ["RowsSpanCellsBatchDevice"]                  # every window of the context: a size query, and no synchronisation on torch's stream
    assert L.log[2][1][8:17] == (8, 101, 102, 0, 0, 2, 1, 0, 0) and [L.log[0][1][8], L.log[1][1][10]] == [2, 2 ** 31 - 1]
    assert L.log[8][1] == (P, P, P, 8, 2, P, P, 2, P, P, 0, P, P, P)
    msg = "encode_pairs_batch_device: L leaves no room for ids, or mode / max_a / stride / max_rows_per_pair are out of range"
    for bad in (dict(L=3), dict(L=8, mode=2), dict(L=8, mode=0, max_a=5), dict(L=8, mode=0, max_a=2, stride=3), dict(L=8, mode=0, max_rows_per_pair=-1)):
        kw = dict(L=bad.pop("L"), cls_id=101, sep_id=102, pad_id=0, **bad)
        raises(ValueError, msg, pairs, 7, d_text, d_off, d_text, d_off, **kw)


def test_encode_packed_and_clm_batch_device(env):
    bf, L, torch = env.bf, env.L, env.torch
    d_text, d_off = dev_docs(torch)
    L.script.update(IdsToPackedRowsBatchDevice=[writes_total(17, 0, 1), 0], IdsToPackedRowsPlanesBatchDevice=[0])
    assert shapes(bf.encode_packed_batch_device(7, d_text, d_off, 4, 101, 102, 0, unk=5)) == DPACK7
    got = bf.encode_packed_batch_device(7, d_text, d_off, 4, 101, None, 0, rows_cap=1, return_offsets=True)
    assert shapes(got) == DPACK7 + [((1, 4), "int32")] * 2
    raises(ValueError, "encode_packed_batch_device: L leaves no room for ids", bf.encode_packed_batch_device, 7, d_text, d_off, 2, 101, 102, 0)
    assert L.log == [("TextToIdsBatchDevice", (P, P, P, 2, 3, P, 4, P, 2, 5, P)), ("IdsToPackedRowsBatchDevice", (P, P, 4, P, 2, 4, 101, 102, 0, 0, N, N, N, N, 0, N, N, P, P)),
                     ("IdsToPackedRowsBatchDevice", (P, P, 4, P, 2, 4, 101, 102, 0, 0, P, P, P, P, 1, P, P, P, P)),
                     ("TextToIdsWithOffsetsBatchDevice", (P, P, P, 2, 3, P, P, P, 6, P, 3, 0, P)),
                     ("IdsToPackedRowsPlanesBatchDevice", (P, P, 6, P, 2, 4, 101, -1, 0, 0, P, P, P, P, 1, P, P, P, 2, P, P, P, P))]
    del L.log[:]
    out = bf.encode_clm_batch_device(7, d_text, d_off, 4, 1, 2, 0, unk=5, drop_last=True, max_ids_per_doc=3)
    assert list(out) == ["input_ids", "seg", "pos", "labels", "row_first_seq", "row_first_pos", "seq_row", "seq_col", "nrows"]
    assert shapes(out.values()) == [((3, 4), "int32")] * 4 + [((3,), "int32")] * 2 + [((2,), "int32")] * 2 + [((2,), "int64")]
    # rows_cap from the size of the tokenizer's id buffer: ceil((6 + 2 * 2) / 4)
    assert L.log == [("TextToIdsBatchDevice", (P, P, P, 2, 3, P, 6, P, 3, 5, P)),
                     ("IdsToStreamRowsBatchDevice", (P, P, 6, P, 2, 4, 1, 2, 0, -100, 1) + (P,) * 6 + (3, P, P, P, P))]


def test_encode_mlm_batch_device(env):
    bf, L, torch = env.bf, env.L, env.torch
    d_text, d_off = dev_docs(torch)
    q = writes_total(17, 0, 1)
    L.script.update(IdsToPackedRowsBatchDevice=[q, 0], IdsToPackedRowsPlanesBatchDevice=[q, 0, q, 0])
    mlm, pmlm = bf.encode_mlm_batch_device, bf.encode_packed_mlm_batch_device
    assert shapes(mlm(7, d_text, d_off, 4, 101, 102, 0, 103, (5, 10), 1)) == [ROWS5[0], ROWS5[1], ROWS5[2], ROWS5[4], ((2, 4), "int32")]
    got = mlm(7, d_text, d_off, 4, 101, 102, 0, 103, (5, 10), 1, whole_word=True, special_ids=[1], max_predictions=2)
    assert shapes(got) == [ROWS5[0], ROWS5[1], ROWS5[2], ROWS5[4]] + [((2, 4), "int32")] * 3 + [((2, 2), "int32")] * 2 + [((2,), "int32")]
    assert shapes(mlm(7, d_text, d_off, 4, 101, None, 0, 103, (5, 10), 1, packed=True)) == DPACK7 + [((1, 4), "int32")]
    assert names(L) == ["TextToIdsBatchDevice", "IdsToRowsBatchDevice", "RowsMlmMaskBatchDevice",
                        "TextToIdsWithOffsetsBatchDevice", "IdsToRowsPlanesBatchDevice", "RowsMlmPredictionsBatchDevice",
                        "TextToIdsBatchDevice", "IdsToPackedRowsBatchDevice", "IdsToPackedRowsBatchDevice", "RowsMlmMaskBatchDevice"]
    # special_ids None: the cls_id, sep_id and pad_id there are
    assert L.log[2][1] == (P, P, 4, 2, P, P, N, N, N, 3, P, 0.15, 0.8, 0.1, 103, 5, 10, -100, 1, 0, P, P, P)
    assert list(ctypes.cast(L.raw[2][1][10], ctypes.POINTER(ctypes.c_int32))[0:3]) == [101, 102, 0]
    assert L.log[5][1] == (P, P, 4, 2, P, P, N, P, P, 1, P, 0.15, 0.8, 0.1, 103, 5, 10, -100, 1, 0, P, P, 2, P, P, P, P)
    assert L.log[9][1] == (P, P, 4, 1, P, N, P, N, N, 2, P, 0.15, 0.8, 0.1, 103, 5, 10, -100, 1, 0, P, P, P)
    assert L.raw[2][1][20] == L.raw[2][1][1]                                # in place: the masked ids are written over the rows
    raises(ValueError, "encode_mlm_batch_device: packed rows have no offset planes, so no whole-word masking", mlm, 7, d_text, d_off, 4, 101, 102, 0, 103, (5, 10), 1,
           whole_word=True, packed=True)
    del L.log[:]
    assert shapes(pmlm(7, d_text, d_off, 4, 101, 102, 0, 103, (5, 10), 1)) == DPACK7 + [((1, 4), "int32")] * 3
    got = pmlm(7, d_text, d_off, 4, None, None, 0, 103, (5, 10), 1, whole_word=False, epoch=4, max_predictions=2)
    assert shapes(got) == DPACK7 + [((1, 4), "int32")] * 3 + [((1, 2), "int32")] * 2 + [((1,), "int32")]
    assert names(L) == ["TextToIdsWithOffsetsBatchDevice", "IdsToPackedRowsPlanesBatchDevice", "IdsToPackedRowsPlanesBatchDevice", "RowsMlmMaskBatchDevice",
                        "TextToIdsWithOffsetsBatchDevice", "IdsToPackedRowsPlanesBatchDevice", "IdsToPackedRowsPlanesBatchDevice", "RowsMlmPredictionsBatchDevice"]
    assert L.log[3][1] == (P, P, 4, 1, P, N, P, P, P, 3, P, 0.15, 0.8, 0.1, 103, 5, 10, -100, 1, 0, P, P, P)
    assert L.log[7][1] == (P, P, 4, 1, P, N, P, N, N, 1, P, 0.15, 0.8, 0.1, 103, 5, 10, -100, 1, 4, P, P, 2, P, P, P, P)
    raises(ValueError, "encode_packed_mlm_batch_device: whole-word masking over packed rows needs cls_id or sep_id (units could join across sequences)",
           pmlm, 7, d_text, d_off, 4, None, None, 0, 103, (5, 10), 1)
    assert "<sync>" not in names(L)


def test_encode_denoise_batch_device(env):
    bf, L, torch = env.bf, env.L, env.torch
    d_text, d_off = dev_docs(torch)
    call = bf.encode_denoise_batch_device
    out = call(7, d_text, d_off, 4, 1, 0, 32099, 5, unk=9, max_ids_per_doc=3)
    assert list(out) == ["input_ids", "labels", "enc_count", "dec_count", "span_count", "rows", "seg", "nrows"]
    assert shapes([out["rows"], out["seg"], out["nrows"]]) == [((2, 4), "int32"), ((2, 4), "int32"), ((1,), "int64")]
    out = call(7, d_text, d_off, 4, 1, 0, 32099, 5, source="rows", start_prob=0.5, special_ids=[3], return_cells=True)
    assert list(out) == ["input_ids", "labels", "enc_count", "dec_count", "span_count", "enc_cells", "dec_cells", "rows", "mask", "nrows"]
    assert shapes([out["rows"], out["mask"], out["nrows"]]) == [((2, 4), "int32"), ((2, 4), "uint8"), ((1,), "int64")]
    p = bf.denoise_start_prob(0.15, 1, 5)
    assert L.log == [("TextToIdsBatchDevice", (P, P, P, 2, 3, P, 6, P, 3, 9, P)),
                     ("IdsToStreamRowsBatchDevice", (P, P, 6, P, 2, 4, -1, 1, 0, -100, 0) + (P,) * 6 + (2, P, P, P, P)),
                     ("RowsDenoiseBatchDevice", (P, P, 4, 2, P, N, P, 2, P, p, 1, 5, 32099, -1, 100, 1, 0, -100, 5, 0, 4, P, N, P, 6, P, N, P, P, P)),
                     ("TextToIdsBatchDevice", (P, P, P, 2, 3, P, 6, P, 3, 0, P)),
                     ("IdsToRowsBatchDevice", (P, P, 6, P, 2, 4, -1, 1, 0, 0, 1, 0, P, P, P, P, 2, P, P)),
                     ("RowsDenoiseBatchDevice", (P, P, 4, 2, P, P, N, 1, P, 0.5, 1, 5, 32099, -1, 100, 1, 0, -100, 5, 0, 4, P, P, P, 6, P, P, P, P, P))]
    assert list(ctypes.cast(L.raw[2][1][8], ctypes.POINTER(ctypes.c_int32))[0:2]) == [0, 1]           # eos_id and pad_id are the special ids
    raises(ValueError, "encode_denoise_batch_device: source is \"stream\" or \"rows\"", call, 7, d_text, d_off, 4, 1, 0, 32099, 5, source="packed")
    raises(ValueError, "encode_denoise_batch_device: eos_id closes every document and is required", call, 7, d_text, d_off, 4, None, 0, 32099, 5)


# ------------------------------------------------------------------------------------------------
# the signature table against the headers
# ------------------------------------------------------------------------------------------------
SCALARS = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64, "uint32_t": ctypes.c_uint32, "double": ctypes.c_double,
           "bool": ctypes.c_bool, "long long": ctypes.c_longlong}


def declarations():
    """{name: (return type, [parameter types])} of every BF_API declaration of the public header and of csrc/bf_internal.h, as C type names with
    `const` and the parameter names dropped; any pointer (or array parameter) is "*" """
    out = {}
    for path in (("include", "blingfiretokdll_amd.h"), ("blingfire_amd", "csrc", "bf_internal.h")):
        src = open(os.path.join(bfutil.ROOT, *path)).read()
        src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
        src = re.sub(r"//[^\n]*", "", src)
        src = "\n".join(l for l in src.splitlines() if not l.lstrip().startswith("#"))
        for ret, name, params in re.findall(r"\bBF_API\s+([^;()]*?)([A-Za-z_][A-Za-z0-9_]*)\s*\(([^;]*?)\)\s*;", src, flags=re.S):
            def ctype(decl, is_param):
                if "*" in decl or "[" in decl:
                    return "*"
                words = [w for w in decl.split() if w != "const"]
                return " ".join(words[:-1] if is_param else words)
            params = " ".join(params.split())
            assert name not in out
            out[name] = (ctype(ret, False), [] if params == "void" else [ctype(p, True) for p in params.split(",")])
    return out


def same_class(c_type, cls):
    if c_type == "*":
        return cls is not None and _is_pointer(cls)
    return cls is SCALARS[c_type]


def test_signature_table_matches_the_headers():
    import blingfire_amd as bf
    decl = declarations()
    public = set(public_symbols())
    assert len(decl) > 70 and public <= set(decl)
    assert public | {"BfSetVariant", "BfSetLexStats", "BfWorkspaceGrows"} <= set(bf._SIGNATURES)
    assert set(bf._SIGNATURES) <= set(decl), "the table names what no header declares: %s" % sorted(set(bf._SIGNATURES) - set(decl))
    for name, (restype, argtypes) in bf._SIGNATURES.items():
        ret, params = decl[name]
        assert same_class(ret, restype), "%s returns %s, bound as %s" % (name, ret, restype)
        assert len(argtypes) == len(params), "%s takes %d parameters, bound with %d" % (name, len(params), len(argtypes))
        for i, (c_type, cls) in enumerate(zip(params, argtypes)):
            assert same_class(c_type, cls), "%s parameter %d is %s, bound as %s" % (name, i, c_type, cls)
    assert bf._SIGNATURES["BfBpeFallbackDocs"][0] is ctypes.c_longlong
    assert bf._SIGNATURES["BfLastError"] == (ctypes.c_char_p, []) and bf._SIGNATURES["GetBlingFireTokVersion"] == (ctypes.c_int, [])


def public_symbols():
    import test_cabi
    return test_cabi.declared_symbols()


def test_bind_applies_the_table():
    import blingfire_amd as bf
    L = bf._bind(StandIn())
    assert set(L.fns) == set(bf._SIGNATURES)
    for name, (restype, argtypes) in bf._SIGNATURES.items():
        assert L.fns[name].restype is restype and L.fns[name].argtypes == argtypes
