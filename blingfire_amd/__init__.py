"""blingfire_amd -- Python mirror of the reference wrapper for the TextToIds path.

Same function names, argument meaning and return conventions as the reference
``dist-pypi/blingfire/__init__.py`` (load_model :229-234, free_model :237-240, text_to_ids :243-253,
change_settings_dummy_prefix :287-288, text_to_words :85-102, text_to_words_with_model :105-122), bound to the MI355X-native ``libblingfiretokdll.so`` built
in-tree by ``blingfire_amd/build.py``.  Additive: ``text_to_ids_batch`` (host buffers) and
``text_to_ids_batch_device`` (torch tensors already resident in HBM).

There is no CPU fallback: if the shared library is missing or no HIP device is visible the calls
raise / return the reference's error value, loudly.
"""
import ctypes
import os
from ctypes import POINTER, byref, c_char_p, c_double, c_float, c_int, c_int32, c_int64, c_uint32, c_uint64, c_void_p

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libblingfiretokdll.so")

_lib = None


def lib():
    """The loaded C-ABI library (built by blingfire_amd/build.py)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("%s is missing: run `python -m blingfire_amd.build` (hipcc, gfx950) first; "
                               "there is no CPU fallback" % LIB_PATH)
        L = ctypes.CDLL(LIB_PATH)
        L.LoadModel.restype = c_void_p
        L.LoadModel.argtypes = [c_char_p]
        L.SetModel.restype = c_void_p
        L.SetModel.argtypes = [c_char_p, c_int]
        L.FreeModel.restype = c_int
        L.FreeModel.argtypes = [c_void_p]
        for name in ("TextToIds", "TextToIds_wp", "TextToIds_sp"):
            f = getattr(L, name)
            f.restype = c_int
            f.argtypes = [c_void_p, c_char_p, c_int, c_void_p, c_int, c_int]
        for name in ("TextToIdsWithOffsets", "TextToIdsWithOffsets_wp", "TextToIdsWithOffsets_sp"):
            f = getattr(L, name)
            f.restype = c_int
            f.argtypes = [c_void_p, c_char_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int]
        L.TextToIdsWithOffsetsBatch.restype = c_int64
        L.TextToIdsWithOffsetsBatch.argtypes = [c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_int, c_int]
        L.TextToIdsWithOffsetsBatchDevice.restype = c_int
        L.TextToIdsWithOffsetsBatchDevice.argtypes = [c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_int64,
                                                      c_void_p, c_int, c_int, c_void_p]
        L.SetNoDummyPrefix.restype = c_int
        L.SetNoDummyPrefix.argtypes = [c_void_p, ctypes.c_bool]
        L.GetBlingFireTokVersion.restype = c_int
        L.TextToIdsBatch.restype = c_int64
        L.TextToIdsBatch.argtypes = [c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int, c_int]
        L.TextToIdsBatchDevice.restype = c_int
        L.TextToIdsBatchDevice.argtypes = [c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_int64, c_void_p,
                                           c_int, c_int, c_void_p]
        L.TextToWords.restype = c_int
        L.TextToWords.argtypes = [c_char_p, c_int, c_void_p, c_int]
        L.TextToWordsWithModel.restype = c_int
        L.TextToWordsWithModel.argtypes = [c_char_p, c_int, c_void_p, c_int, c_void_p]
        L.TextToWordsWithOffsets.restype = c_int
        L.TextToWordsWithOffsets.argtypes = [c_char_p, c_int, c_void_p, c_void_p, c_void_p, c_int]
        L.TextToWordsWithOffsetsWithModel.restype = c_int
        L.TextToWordsWithOffsetsWithModel.argtypes = [c_char_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p]
        L.TextToSentences.restype = c_int
        L.TextToSentences.argtypes = [c_char_p, c_int, c_void_p, c_int]
        L.TextToSentencesWithModel.restype = c_int
        L.TextToSentencesWithModel.argtypes = [c_char_p, c_int, c_void_p, c_int, c_void_p]
        L.TextToSentencesWithOffsets.restype = c_int
        L.TextToSentencesWithOffsets.argtypes = [c_char_p, c_int, c_void_p, c_void_p, c_void_p, c_int]
        L.TextToSentencesWithOffsetsWithModel.restype = c_int
        L.TextToSentencesWithOffsetsWithModel.argtypes = [c_char_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p]
        L.TextToWordsBatch.restype = c_int64
        L.TextToWordsBatch.argtypes = [c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_void_p]
        L.TextToWordsBatchDevice.restype = c_int
        L.TextToWordsBatchDevice.argtypes = [c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_int64, c_void_p, c_void_p]
        L.TextToSentencesBatch.restype = c_int64
        L.TextToSentencesBatch.argtypes = [c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_void_p]
        L.TextToSentencesBatchDevice.restype = c_int
        L.TextToSentencesBatchDevice.argtypes = [c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_int64, c_void_p, c_void_p]
        L.IdsToText.restype = c_int
        L.IdsToText.argtypes = [c_void_p, c_void_p, c_int, c_void_p, c_int, ctypes.c_bool]
        L.IdsToTextBatch.restype = c_int64
        L.IdsToTextBatch.argtypes = [c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int]
        L.IdsToTextBatchDevice.restype = c_int
        L.IdsToTextBatchDevice.argtypes = [c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int, c_void_p]
        L.IdsToRowsBatch.restype = c_int64
        L.IdsToRowsBatch.argtypes = [c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int, c_int, c_int, c_int, c_int, c_int,
                                     c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p]
        L.IdsToRowsBatchDevice.restype = c_int
        L.IdsToRowsBatchDevice.argtypes = [c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_int, c_int, c_int, c_int, c_int, c_int, c_int,
                                           c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p]
        L.IdsToPairRowsBatch.restype = c_int64
        L.IdsToPairRowsBatch.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64] + [c_int] * 9 + [c_void_p] * 5 + [c_int64, c_void_p]
        L.IdsToPairRowsBatchDevice.restype = c_int
        L.IdsToPairRowsBatchDevice.argtypes = [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_void_p, c_int64] + [c_int] * 9 + [c_void_p] * 5 + [
            c_int64, c_void_p, c_void_p]
        L.IdsToRowsPlanesBatch.restype = c_int64
        L.IdsToRowsPlanesBatch.argtypes = L.IdsToRowsBatch.argtypes + [c_int, c_void_p, c_void_p, c_void_p]
        L.IdsToRowsPlanesBatchDevice.restype = c_int
        L.IdsToRowsPlanesBatchDevice.argtypes = L.IdsToRowsBatchDevice.argtypes[:-1] + [c_int, c_void_p, c_void_p, c_void_p, c_void_p]
        L.IdsToPairRowsPlanesBatch.restype = c_int64
        L.IdsToPairRowsPlanesBatch.argtypes = L.IdsToPairRowsBatch.argtypes + [c_int, c_void_p, c_void_p, c_void_p, c_void_p]
        L.IdsToPairRowsPlanesBatchDevice.restype = c_int
        L.IdsToPairRowsPlanesBatchDevice.argtypes = L.IdsToPairRowsBatchDevice.argtypes[:-1] + [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]
        L.RowsSpanCellsBatchDevice.restype = c_int
        L.RowsSpanCellsBatchDevice.argtypes = [c_void_p, c_void_p, c_void_p, c_int, c_int64, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int,
                                               c_void_p, c_void_p, c_void_p]
        L.RowsMlmMaskBatchDevice.restype = c_int
        L.RowsMlmMaskBatchDevice.argtypes = [c_void_p, c_void_p, c_int, c_int64] + [c_void_p] * 5 + [c_int, c_void_p] + [c_double] * 3 + [c_int] * 4 + [
            c_uint64, c_uint32, c_void_p, c_void_p, c_void_p]
        L.RowsMlmPredictionsBatchDevice.restype = c_int
        L.RowsMlmPredictionsBatchDevice.argtypes = L.RowsMlmMaskBatchDevice.argtypes[:-1] + [c_int, c_void_p, c_void_p, c_void_p, c_void_p]
        L.RowsDenoiseBatchDevice.restype = c_int
        L.RowsDenoiseBatchDevice.argtypes = [c_void_p, c_void_p, c_int, c_int64] + [c_void_p] * 3 + [c_int, c_void_p, c_double] + [c_int] * 8 + [c_uint64, c_uint32] + [
            c_int, c_void_p, c_void_p, c_void_p] * 2 + [c_void_p, c_void_p]
        L.IdsToPackedRowsBatch.restype = c_int64
        L.IdsToPackedRowsBatch.argtypes = [c_void_p, c_void_p, c_void_p, c_int64] + [c_int] * 5 + [c_void_p] * 4 + [c_int64, c_void_p, c_void_p]
        L.IdsToPackedRowsBatchDevice.restype = c_int
        L.IdsToPackedRowsBatchDevice.argtypes = [c_void_p, c_void_p, c_int64, c_void_p, c_int64] + [c_int] * 5 + [c_void_p] * 4 + [c_int64] + [c_void_p] * 4
        L.IdsToPackedRowsPlanesBatch.restype = c_int64
        L.IdsToPackedRowsPlanesBatch.argtypes = L.IdsToPackedRowsBatch.argtypes + [c_int, c_void_p, c_void_p, c_void_p]
        L.IdsToPackedRowsPlanesBatchDevice.restype = c_int
        L.IdsToPackedRowsPlanesBatchDevice.argtypes = L.IdsToPackedRowsBatchDevice.argtypes[:-1] + [c_int, c_void_p, c_void_p, c_void_p, c_void_p]
        L.IdsToStreamRowsBatch.restype = c_int64
        L.IdsToStreamRowsBatch.argtypes = [c_void_p, c_void_p, c_void_p, c_int64] + [c_int] * 6 + [c_void_p] * 6 + [c_int64, c_void_p, c_void_p]
        L.IdsToStreamRowsBatchDevice.restype = c_int
        L.IdsToStreamRowsBatchDevice.argtypes = [c_void_p, c_void_p, c_int64, c_void_p, c_int64] + [c_int] * 6 + [c_void_p] * 6 + [c_int64] + [c_void_p] * 4
        L.BfLastKernelMs.restype = c_int
        L.BfLastKernelMs.argtypes = [c_void_p, POINTER(c_float), c_int]
        L.BfLastStatus.restype = c_int
        L.BfLastStatus.argtypes = [c_void_p]
        L.BfLastError.restype = c_char_p
        L.BfModelKind.restype = c_int
        L.BfModelKind.argtypes = [c_void_p]
        L.BfSetVariant.restype = c_int
        L.BfSetVariant.argtypes = [c_void_p, c_int]
        L.DictGetInfoBatch.restype = c_int64
        L.DictGetInfoBatch.argtypes = [c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int64, c_void_p]
        L.DictGetInfoBatchDevice.restype = c_int
        L.DictGetInfoBatchDevice.argtypes = [c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p]
        L.BfSetDevices.restype = c_int
        L.BfSetDevices.argtypes = [c_void_p, c_void_p, c_int]
        L.BfShardHandle.restype = c_void_p
        L.BfShardHandle.argtypes = [c_void_p, c_int]
        L.BfShardRanges.restype = c_int
        L.BfShardRanges.argtypes = [c_void_p, c_int64, c_int, c_void_p]
        L.BfSetLexStats.restype = c_int
        L.BfSetLexStats.argtypes = [c_void_p, c_int]
        L.BfSetBpePoolBytes.restype = c_int64
        L.BfSetBpePoolBytes.argtypes = [c_void_p, c_int64]
        L.BfWorkspaceGrows.restype = c_int
        L.BfWorkspaceGrows.argtypes = [c_void_p]
        L.BfReserve.restype = c_int
        L.BfReserve.argtypes = [c_void_p, c_int64, c_int64, c_int]
        L.NormalizeSpaces.restype = c_int
        L.NormalizeSpaces.argtypes = [c_char_p, c_int, c_void_p, c_int, c_int]
        L.TextToHashes.restype = c_int
        L.TextToHashes.argtypes = [c_char_p, c_int, c_void_p, c_int, c_int, c_int]
        L.WordHyphenationWithModel.restype = c_int
        L.WordHyphenationWithModel.argtypes = [c_char_p, c_int, c_void_p, c_int, c_void_p, c_int]
        L.WordHyphenationBatch.restype = c_int64
        L.WordHyphenationBatch.argtypes = [c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int]
        L.WordHyphenationBatchDevice.restype = c_int
        L.WordHyphenationBatchDevice.argtypes = [c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_int64, c_void_p, c_int, c_void_p]
        _lib = L
    return _lib


def get_blingfiretok_version():
    return lib().GetBlingFireTokVersion()


def load_model(file_name):
    """reference __init__.py:229-234; raises instead of returning a NULL handle."""
    h = lib().LoadModel(file_name.encode("utf-8"))
    if not h:
        raise RuntimeError("LoadModel(%r) failed: %s" % (file_name, lib().BfLastError().decode("utf-8", "replace")))
    return h


def free_model(h):
    lib().FreeModel(c_void_p(h))


def text_to_ids(h, s, max_len, unk=0, no_padding=False):
    """reference __init__.py:243-253: zero-padded uint32 array of max_len (or the exact count with no_padding)."""
    s_bytes = s.encode("utf-8") if isinstance(s, str) else bytes(s)
    o = (c_int32 * max_len)()
    t = lib().TextToIds(c_void_p(h), s_bytes, len(s_bytes), byref(o), max_len, unk)
    n = min(max_len, t) if no_padding else max_len
    return np.frombuffer(o, dtype=np.uint32, count=n)


def utf8text_to_ids_with_offsets(h, s_bytes, max_len, unk=0, no_padding=False):
    """reference __init__.py:272-284: (ids uint32, start offsets int32, end offsets int32), zero padded to max_len."""
    o = (c_int32 * max_len)()
    o_s = (c_int32 * max_len)()
    o_e = (c_int32 * max_len)()
    t = lib().TextToIdsWithOffsets(c_void_p(h), s_bytes, len(s_bytes), byref(o), byref(o_s), byref(o_e), max_len, unk)
    n = min(max_len, t) if no_padding else max_len
    return (np.frombuffer(o, dtype=np.uint32, count=n), np.frombuffer(o_s, dtype=np.int32, count=n),
            np.frombuffer(o_e, dtype=np.int32, count=n))


def normalize_spaces(s, uSpace=0x20):
    """reference __init__.py:65-82: runs of white space -> one uSpace, leading / trailing dropped; '' on error."""
    s_bytes = s.encode("utf-8")
    o = ctypes.create_string_buffer(len(s_bytes) * 2 + 4)
    n = lib().NormalizeSpaces(s_bytes, len(s_bytes), o, len(o), uSpace)
    return "" if n == -1 or n > len(o) else o.value.decode("utf-8")


def text_to_hashes(s, word_n_grams, bucketSize):
    """reference __init__.py:151-167: int32 array of the token hashes followed by the word n-gram hashes; '' on error."""
    s_bytes = s.encode("utf-8")
    cap = max(word_n_grams * len(s_bytes), 1)
    o = (c_int32 * cap)()
    n = lib().TextToHashes(s_bytes, len(s_bytes), byref(o), cap, word_n_grams, bucketSize)
    if n == -1 or n > cap:
        return ""
    return np.frombuffer(o, dtype=np.int32, count=n)


def word_hyphenation_with_model(h, s, uHy=0x2D):
    """reference __init__.py:125-142: the word with uHy behind every hyphenation point of the model's [w2h] patterns (h: a handle of
    syllab.bin or of another model with that section); '' on error or for a handle without one."""
    s_bytes = s.encode("utf-8")
    o = ctypes.create_string_buffer(len(s_bytes) * 4 + 1)
    n = lib().WordHyphenationWithModel(s_bytes, len(s_bytes), o, len(o), c_void_p(h) if h else None, uHy)
    return "" if n == -1 or n > len(o) else o.value.decode("utf-8")


def word_hyphenation_batch(h, words, uHy=0x2D):
    """additive: word_hyphenation_with_model over many words (str or bytes) in one call -> list of str; '' where the single call fails."""
    text, off = pack_docs([w.encode("utf-8") if isinstance(w, str) else bytes(w) for w in words])
    nw = len(off) - 1
    t_off = np.zeros(nw + 1, dtype=np.int64)
    args = (c_void_p(h), c_void_p(text.ctypes.data), c_void_p(off.ctypes.data), nw)
    fn = lib().WordHyphenationBatch
    n = fn(*args, None, 0, c_void_p(t_off.ctypes.data), uHy)
    out = np.empty(0, dtype=np.uint8)
    if n == -3:                                           # BF_E_CAPACITY: the offsets tell the size
        out = np.empty(int(t_off[-1]), dtype=np.uint8)
        n = fn(*args, c_void_p(out.ctypes.data), len(out), c_void_p(t_off.ctypes.data), uHy)
    if n < 0:
        raise RuntimeError("WordHyphenationBatch failed: %d (%s)" % (n, lib().BfLastError().decode("utf-8", "replace")))
    raw = out.tobytes()
    return [raw[t_off[i]:t_off[i + 1]].decode("utf-8") for i in range(nw)]


def text_to_words(s):
    """reference __init__.py:85-102: space-joined words by the built-in wbd.bin; '' on error."""
    s_bytes = s.encode("utf-8")
    o = ctypes.create_string_buffer(len(s_bytes) * 3)
    n = lib().TextToWords(s_bytes, len(s_bytes), o, len(o))
    return "" if n == -1 or n > len(o) else o.value.decode("utf-8")


def text_to_words_with_model(h, s):
    """reference __init__.py:105-122"""
    s_bytes = s.encode("utf-8")
    o = ctypes.create_string_buffer(len(s_bytes) * 3)
    n = lib().TextToWordsWithModel(s_bytes, len(s_bytes), o, len(o), c_void_p(h))
    return "" if n == -1 or n > len(o) else o.value.decode("utf-8")


def text_to_words_with_offsets(s, h=None):
    """reference __init__.py:161-223: (string, [(begin, end) per word]) as character offsets into `s`, end exclusive."""
    s_bytes = s.encode("utf-8")
    cap = len(s_bytes) * 3
    o = ctypes.create_string_buffer(max(cap, 1))
    st = (c_int32 * max(cap, 1))()
    en = (c_int32 * max(cap, 1))()
    n = lib().TextToWordsWithOffsetsWithModel(s_bytes, len(s_bytes), o, byref(st), byref(en), cap, c_void_p(h) if h else None)
    if n == -1 or n > cap:
        return "", []
    words = o.value.decode("utf-8")
    k = len(words.split(" ")) if words else 0
    lead = np.frombuffer(s_bytes, dtype=np.uint8) & 0xC0 != 0x80
    char_at = np.concatenate([[0], np.cumsum(lead)])          # byte offset -> number of characters that start before it
    return words, [(int(char_at[st[i]]), int(char_at[en[i] + 1])) for i in range(k)]


def text_to_sentences(s):
    """reference __init__.py:45-62: one sentence per line by the built-in sbd.bin; '' on error."""
    s_bytes = s.encode("utf-8")
    o = ctypes.create_string_buffer(len(s_bytes) * 2)
    n = lib().TextToSentences(s_bytes, len(s_bytes), o, len(o))
    return "" if n == -1 or n > len(o) else o.value.decode("utf-8")


def text_to_sentences_with_model(h, s):
    """reference __init__.py:65-82"""
    s_bytes = s.encode("utf-8")
    o = ctypes.create_string_buffer(len(s_bytes) * 2)
    n = lib().TextToSentencesWithModel(s_bytes, len(s_bytes), o, len(o), c_void_p(h))
    return "" if n == -1 or n > len(o) else o.value.decode("utf-8")


def text_to_sentences_and_offsets(s, h=None):
    """reference __init__.py:225-226: (string, [(begin, end) per sentence]) as character offsets into `s`, end exclusive."""
    s_bytes = s.encode("utf-8")
    cap = len(s_bytes) * 2
    o = ctypes.create_string_buffer(max(cap, 1))
    st = (c_int32 * max(cap, 1))()
    en = (c_int32 * max(cap, 1))()
    n = lib().TextToSentencesWithOffsetsWithModel(s_bytes, len(s_bytes), o, byref(st), byref(en), cap, c_void_p(h) if h else None)
    if n == -1 or n > cap:
        return "", []
    sents = o.value.decode("utf-8")
    k = sents.count("\n") + 1 if sents else 0
    lead = np.frombuffer(s_bytes, dtype=np.uint8) & 0xC0 != 0x80
    char_at = np.concatenate([[0], np.cumsum(lead)])
    return sents, [(int(char_at[st[i]]), int(char_at[en[i] + 1])) for i in range(k)]


def text_to_sentences_batch(docs, h=None):
    """additive: TextToSentences over many documents; h None = the built-in sbd.bin.  Same conventions as text_to_words_batch."""
    return text_to_words_batch(docs, h, _fn="TextToSentencesBatch")


def text_to_words_batch(docs, h=None, _fn="TextToWordsBatch"):
    """additive: TextToWords over many documents (list of bytes, or a (text uint8, offsets int64) pair) -> (text uint8, offsets int64[ndocs+1]);
    h None = the built-in wbd.bin."""
    text, off = docs if isinstance(docs, tuple) else pack_docs(docs)
    text = np.ascontiguousarray(text, dtype=np.uint8); off = np.ascontiguousarray(off, dtype=np.int64)
    nd = len(off) - 1
    t_off = np.zeros(nd + 1, dtype=np.int64)
    hp = c_void_p(h) if h else None
    fn = getattr(lib(), _fn)
    n = fn(hp, c_void_p(text.ctypes.data), c_void_p(off.ctypes.data), nd, None, 0, c_void_p(t_off.ctypes.data))
    out = np.empty(0, dtype=np.uint8)
    if n == -3:                                           # BF_E_CAPACITY: the offsets tell the size
        out = np.empty(int(t_off[-1]), dtype=np.uint8)
        n = fn(hp, c_void_p(text.ctypes.data), c_void_p(off.ctypes.data), nd, c_void_p(out.ctypes.data), len(out), c_void_p(t_off.ctypes.data))
    if n < 0:
        raise RuntimeError("%s failed: %d (%s)" % (_fn, n, lib().BfLastError().decode("utf-8", "replace")))
    return out, t_off


def ids_to_text(h, ids, skip_special_tokens=True, output_buffer_size=None):
    """reference __init__.py:256-269: text of an id array (numpy int32 / uint32); '' on error or if the buffer is too small."""
    ids = np.ascontiguousarray(ids).view(np.int32) if isinstance(ids, np.ndarray) and ids.dtype.itemsize == 4 else np.asarray(ids, dtype=np.int32)
    if output_buffer_size is None:
        output_buffer_size = len(ids) * 32
    o = ctypes.create_string_buffer(max(output_buffer_size, 1))
    n = lib().IdsToText(c_void_p(h), c_void_p(ids.ctypes.data), len(ids), o, output_buffer_size, bool(skip_special_tokens))
    if n == -1 or n > output_buffer_size:
        return ""
    return o.value.decode("utf-8")


def ids_to_text_batch(h, ids, id_off, skip_special_tokens=True):
    """additive: (text bytes as uint8 array, text offsets int64[nseq+1]) for many id sequences at once (IdsToTextBatch)."""
    ids = np.ascontiguousarray(ids, dtype=np.int32)
    id_off = np.ascontiguousarray(id_off, dtype=np.int64)
    nseq = len(id_off) - 1
    t_off = np.zeros(nseq + 1, dtype=np.int64)
    n = lib().IdsToTextBatch(c_void_p(h), c_void_p(ids.ctypes.data), c_void_p(id_off.ctypes.data), nseq, None, 0, c_void_p(t_off.ctypes.data),
                             int(bool(skip_special_tokens)))
    if n == -3:                                           # BF_E_CAPACITY: the offsets tell the size
        text = np.empty(int(t_off[-1]), dtype=np.uint8)
        n = lib().IdsToTextBatch(c_void_p(h), c_void_p(ids.ctypes.data), c_void_p(id_off.ctypes.data), nseq, c_void_p(text.ctypes.data), len(text),
                                 c_void_p(t_off.ctypes.data), int(bool(skip_special_tokens)))
    else:
        text = np.empty(0, dtype=np.uint8)
    if n < 0:
        raise RuntimeError("IdsToTextBatch failed: %d (%s)" % (n, lib().BfLastError().decode("utf-8", "replace")))
    return text, t_off


def change_settings_dummy_prefix(h, add_prefix):
    lib().SetNoDummyPrefix(c_void_p(h), bool(not add_prefix))


# ---------------------------------------------------------------------------------------------
# additive batch API
# ---------------------------------------------------------------------------------------------

def pack_docs(docs):
    """list of str/bytes -> (uint8 array, int64 offsets[ndocs+1])"""
    bs = [d.encode("utf-8") if isinstance(d, str) else bytes(d) for d in docs]
    off = np.zeros(len(bs) + 1, dtype=np.int64)
    if bs:
        np.cumsum([len(b) for b in bs], out=off[1:])
    text = np.frombuffer(b"".join(bs), dtype=np.uint8) if bs else np.zeros(0, dtype=np.uint8)
    return text, off


def set_devices(h, device_ids):
    """Range-shards the host-buffer batch calls of h over the listed devices of this node (BfSetDevices: tables replicated, contiguous
    byte-balanced document ranges, one host thread per device, no collective).  A device may be listed more than once."""
    arr = (c_int * len(device_ids))(*[int(d) for d in device_ids])
    r = lib().BfSetDevices(c_void_p(h), arr, len(device_ids))
    if r != 0:
        raise RuntimeError("BfSetDevices failed (%d): %s" % (r, lib().BfLastError().decode("utf-8", "replace")))


def shard_handle(h, g):
    """the handle that tokenises range g after set_devices (None past the last range); owned by h"""
    return lib().BfShardHandle(c_void_p(h), int(g))


def shard_ranges(doc_offsets, G):
    """document ranges a batch is split into over G devices: int64[G + 1] (BfShardRanges; no device needed)"""
    off = np.ascontiguousarray(doc_offsets, dtype=np.int64)
    bounds = np.zeros(G + 1, dtype=np.int64)
    r = lib().BfShardRanges(off.ctypes.data, len(off) - 1, G, bounds.ctypes.data)
    if r != 0:
        raise RuntimeError("BfShardRanges failed (%d)" % r)
    return bounds


def text_to_ids_batch(h, docs, max_len, unk=0):
    """For every document exactly what TextToIds(h, doc, len, buf, max_len, unk) writes, concatenated.

    docs: list of str/bytes, or a (uint8 ndarray, int64 offsets) pair.  Returns (ids int32[total], offsets int64[ndocs+1]).
    """
    text, off = docs if isinstance(docs, tuple) else pack_docs(docs)
    text = np.ascontiguousarray(text, dtype=np.uint8)
    off = np.ascontiguousarray(off, dtype=np.int64)
    ndocs = len(off) - 1
    total = int(off[-1] - off[0]) if ndocs > 0 else 0
    cap = min(2 * (total + ndocs), ndocs * max(max_len, 0)) + 1      # every id covers >= 1 element of <= 2*(n+1) per document
    ids = np.empty(cap, dtype=np.int32)
    id_off = np.zeros(ndocs + 1, dtype=np.int64)
    r = lib().TextToIdsBatch(c_void_p(h), text.ctypes.data, off.ctypes.data, ndocs, ids.ctypes.data, cap, id_off.ctypes.data,
                             max_len, unk)
    if r < 0:
        raise RuntimeError("TextToIdsBatch failed (%d): %s" % (r, lib().BfLastError().decode("utf-8", "replace")))
    return ids[:r], id_off


def text_to_ids_with_offsets_batch(h, docs, max_len, unk=0):
    """Batch form of TextToIdsWithOffsets: (ids, starts, ends, id_offsets); starts/ends are byte offsets inside each document."""
    text, off = docs if isinstance(docs, tuple) else pack_docs(docs)
    text = np.ascontiguousarray(text, dtype=np.uint8)
    off = np.ascontiguousarray(off, dtype=np.int64)
    ndocs = len(off) - 1
    total = int(off[-1] - off[0]) if ndocs > 0 else 0
    cap = min(2 * (total + ndocs), ndocs * max(max_len, 0)) + 1
    ids = np.empty(cap, dtype=np.int32)
    starts = np.empty(cap, dtype=np.int32)
    ends = np.empty(cap, dtype=np.int32)
    id_off = np.zeros(ndocs + 1, dtype=np.int64)
    r = lib().TextToIdsWithOffsetsBatch(c_void_p(h), text.ctypes.data, off.ctypes.data, ndocs, ids.ctypes.data, starts.ctypes.data,
                                        ends.ctypes.data, cap, id_off.ctypes.data, max_len, unk)
    if r < 0:
        raise RuntimeError("TextToIdsWithOffsetsBatch failed (%d): %s" % (r, lib().BfLastError().decode("utf-8", "replace")))
    return ids[:r], starts[:r], ends[:r], id_off


def text_to_ids_batch_device(h, d_text, d_doc_off, max_len, unk=0, out_ids=None, out_off=None, stream=None):
    """Device-resident batch: torch uint8 text tensor + int64 offsets tensor (both on the model's GPU).

    Enqueues on torch's current stream (or `stream`) and returns (ids int32[cap], id_offsets int64[ndocs+1]) tensors
    without synchronising; the valid id count is id_offsets[-1].
    """
    import torch
    ndocs = d_doc_off.numel() - 1
    total = d_text.numel()
    cap = max(1, min(2 * (total + ndocs), ndocs * max(max_len, 0)))
    if out_ids is None:
        out_ids = torch.empty(cap, dtype=torch.int32, device=d_text.device)
    if out_off is None:
        out_off = torch.empty(ndocs + 1, dtype=torch.int64, device=d_text.device)
    s = stream if stream is not None else torch.cuda.current_stream(d_text.device).cuda_stream
    r = lib().TextToIdsBatchDevice(c_void_p(h), d_text.data_ptr(), d_doc_off.data_ptr(), ndocs, total, out_ids.data_ptr(),
                                   out_ids.numel(), out_off.data_ptr(), max_len, unk, c_void_p(s))
    if r != 0:
        raise RuntimeError("TextToIdsBatchDevice failed (%d): %s" % (r, lib().BfLastError().decode("utf-8", "replace")))
    return out_ids, out_off


def text_to_ids_with_offsets_batch_device(h, d_text, d_doc_off, max_len, unk=0, stream=None):
    """Device-resident text_to_ids_with_offsets_batch, the mirror of text_to_ids_batch_device: (ids int32[cap], starts int32[cap],
    ends int32[cap], id_offsets int64[ndocs+1]) tensors, enqueued without synchronising; starts / ends are byte offsets inside each
    document (the end inclusive), the valid count is id_offsets[-1]."""
    import torch
    ndocs = d_doc_off.numel() - 1
    total = d_text.numel()
    cap = max(1, min(2 * (total + ndocs), ndocs * max(max_len, 0)))
    ids, starts, ends = (torch.empty(cap, dtype=torch.int32, device=d_text.device) for _ in range(3))
    out_off = torch.empty(ndocs + 1, dtype=torch.int64, device=d_text.device)
    s = stream if stream is not None else torch.cuda.current_stream(d_text.device).cuda_stream
    r = lib().TextToIdsWithOffsetsBatchDevice(c_void_p(h), d_text.data_ptr(), d_doc_off.data_ptr(), ndocs, total, ids.data_ptr(), starts.data_ptr(),
                                              ends.data_ptr(), cap, out_off.data_ptr(), max_len, unk, c_void_p(s))
    if r != 0:
        raise RuntimeError("TextToIdsWithOffsetsBatchDevice failed (%d): %s" % (r, lib().BfLastError().decode("utf-8", "replace")))
    return ids, starts, ends, out_off


def ids_to_text_batch_device(h, d_ids, d_id_off, out_text=None, out_off=None, skip_special_tokens=True, stream=None):
    """Device-resident IdsToText: torch int32 ids + int64 offsets on the model's GPU -> (text uint8[cap], text offsets int64[nseq+1]).
    Without `out_text` a buffer of 16 bytes per id is used (IdsToTextBatchDevice never writes past it)."""
    import torch
    nseq = d_id_off.numel() - 1
    if out_text is None:
        out_text = torch.empty(max(16 * d_ids.numel(), 1), dtype=torch.uint8, device=d_ids.device)
    if out_off is None:
        out_off = torch.empty(nseq + 1, dtype=torch.int64, device=d_ids.device)
    s = stream if stream is not None else torch.cuda.current_stream(d_ids.device).cuda_stream
    r = lib().IdsToTextBatchDevice(c_void_p(h), d_ids.data_ptr(), d_id_off.data_ptr(), nseq, out_text.data_ptr(), out_text.numel(),
                                   out_off.data_ptr(), int(bool(skip_special_tokens)), c_void_p(s))
    if r != 0:
        raise RuntimeError("IdsToTextBatchDevice failed (%d): %s" % (r, lib().BfLastError().decode("utf-8", "replace")))
    return out_text, out_off


def _special(i):
    return -1 if i is None else int(i)


def _plane_tail(srcs, fill, addr):
    """the companion-plane arguments of the ...Planes calls: `srcs` = one list of arrays / tensors (None entries allowed) per side, `fill` = one int per
    plane, addr(x) = the address of an array.  -> (nplanes, tail) with tail(outs) = the arguments for the plane outputs `outs` (None: every
    plane NULL); the ctypes arrays live as long as `tail` does"""
    n = len(fill)
    if n > 4 or any(len(side) != n for side in srcs):
        raise ValueError("companion planes: at most 4, and one source (or None) per fill value and side")
    c_src = [(c_void_p * max(n, 1))(*[None if x is None else addr(x) for x in side]) for side in srcs]
    c_fill = (c_int32 * max(n, 1))(*[int(f) for f in fill])

    def tail(outs):
        c_out = (c_void_p * max(n, 1))(*([None] * n if outs is None else [addr(o) for o in outs]))
        return (n, *c_src, c_fill, c_out)
    return n, tail


def _rows_host(name, pre, nseq, L, planes, extra=None):
    """the host forms of the row stage: the size query, then every output (one `planes` dtype per [R, L] plane, row item, row first id).
    extra = (nplanes, tail) of _plane_tail: the ...Planes calls, whose int32 [R, L] planes are appended to the result as a list"""
    fn = getattr(lib(), name)
    nextra, tail = extra if extra else (0, lambda outs: ())
    r_off = np.zeros(nseq + 1, dtype=np.int64)
    n = fn(*pre, *[None] * (len(planes) + 2), 0, r_off.ctypes.data, *tail(None))
    if n < 0:
        raise RuntimeError("%s failed: %d (%s)" % (name, n, lib().BfLastError().decode("utf-8", "replace")))
    outs = [np.empty((n, L), dtype=t) for t in planes] + [np.empty(n, dtype=np.int32), np.empty(n, dtype=np.int32)]
    more = [np.empty((n, L), dtype=np.int32) for _ in range(nextra)]
    if n > 0:
        r = fn(*pre, *[o.ctypes.data for o in outs], n, r_off.ctypes.data, *tail(more))
        if r != n:
            raise RuntimeError("%s failed: %d (%s)" % (name, r, lib().BfLastError().decode("utf-8", "replace")))
    return (*outs, r_off, more) if extra else (*outs, r_off)


def _rows_device(name, pre, nseq, L, planes, one_row, rows_cap, dev, stream, extra=None):
    """the device forms of the row stage.  rows_cap None: nseq rows where one row per item is certain (`one_row`), else a size query whose
    total is read back.  extra: as in _rows_host"""
    import torch
    fn = getattr(lib(), name)
    nextra, tail = extra if extra else (0, lambda outs: ())
    s = c_void_p(stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream)
    r_off = torch.empty(nseq + 1, dtype=torch.int64, device=dev)

    def call(outs, cap, more=None):
        r = fn(*pre, *outs, cap, r_off.data_ptr(), *tail(more), s)
        if r != 0:
            raise RuntimeError("%s failed (%d): %s" % (name, r, lib().BfLastError().decode("utf-8", "replace")))
    if rows_cap is None:
        if one_row:
            rows_cap = nseq
        else:
            call([None] * (len(planes) + 2), 0)
            if stream is not None:
                torch.cuda.synchronize(dev)               # (a raw stream handle: nothing finer to wait on)
            rows_cap = int(r_off[-1].item())
    outs = [torch.empty((rows_cap, L), dtype=t, device=dev) for t in planes] + [torch.empty(rows_cap, dtype=torch.int32, device=dev) for _ in range(2)]
    more = [torch.empty((rows_cap, L), dtype=torch.int32, device=dev) for _ in range(nextra)]
    call([o.data_ptr() for o in outs], rows_cap, more)
    return (*outs, r_off, more) if extra else (*outs, r_off)


def ids_to_rows_batch(h, ids, id_off, L, cls_id=None, sep_id=None, pad_id=0, stride=0, max_rows_per_seq=1, pad_left=False):
    """additive: ragged ids (int32 array + int64 offsets[nseq+1]) -> fixed-shape model inputs (IdsToRowsBatch).  A sequence longer than
    the row is cut into windows that share `stride` ids (max_rows_per_seq: 1 = truncate, 0 = every window); cls_id / sep_id None = no
    such special.  Returns (rows int32[R, L], mask uint8[R, L], row_seq int32[R], row_first int32[R], row_offsets int64[nseq+1]):
    the rows of sequence q are [row_offsets[q], row_offsets[q+1]), row_first is the index within its sequence of a row's first id."""
    ids = np.ascontiguousarray(ids, dtype=np.int32)
    id_off = np.ascontiguousarray(id_off, dtype=np.int64)
    nseq = len(id_off) - 1
    pre = (c_void_p(h), ids.ctypes.data, id_off.ctypes.data, nseq, int(L), _special(cls_id), _special(sep_id), int(pad_id), int(stride),
           int(max_rows_per_seq), int(bool(pad_left)))
    return _rows_host("IdsToRowsBatch", pre, nseq, L, (np.int32, np.uint8))


def ids_to_rows_batch_device(h, d_ids, d_id_off, L, cls_id=None, sep_id=None, pad_id=0, stride=0, max_rows_per_seq=1, pad_left=False,
                             rows_cap=None, stream=None):
    """Device-resident ids_to_rows_batch: torch int32 ids + int64 offsets on one GPU (text_to_ids_batch_device's results as they are) ->
    the same five results as tensors on that device, enqueued on torch's current stream (or `stream`).  rows_cap None: nseq rows when
    max_rows_per_seq is 1 (nothing is read back); otherwise a size query whose total is read back (one synchronisation).  With a
    rows_cap of the caller's the tensors have rows_cap rows, row_offsets[-1] of them valid; rows beyond it are dropped (BfLastStatus bit 0)."""
    import torch
    nseq = d_id_off.numel() - 1
    pre = (c_void_p(h), d_ids.data_ptr(), d_ids.numel(), d_id_off.data_ptr(), nseq, int(L), _special(cls_id), _special(sep_id), int(pad_id),
           int(stride), int(max_rows_per_seq), int(bool(pad_left)))
    return _rows_device("IdsToRowsBatchDevice", pre, nseq, L, (torch.int32, torch.uint8), max_rows_per_seq == 1, rows_cap, d_ids.device, stream)


def _np_i32(x):
    return None if x is None else np.ascontiguousarray(x, dtype=np.int32)


def _dev_i32(t, dev, what):
    """a device array a kernel reads as int32 through its address: None, or a contiguous torch.int32 tensor on `dev` (anything else would be read
    as garbage -- an int64 labels tensor as pairs of int32 -- so it is refused, not converted behind the caller's back)"""
    import torch
    if t is None:
        return None
    if not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or not t.is_contiguous() or t.device != dev:
        raise ValueError("%s must be a contiguous torch.int32 tensor on %s (got %s)" % (
            what, dev, "%s, %s, %s" % (t.dtype, t.device, "contiguous" if t.is_contiguous() else "not contiguous") if isinstance(t, torch.Tensor) else type(t).__name__))
    return t


def ids_to_rows_planes_batch(h, ids, id_off, L, cls_id=None, sep_id=None, pad_id=0, stride=0, max_rows_per_seq=1, pad_left=False, src=(), fill=()):
    """ids_to_rows_batch with companion planes (IdsToRowsPlanesBatch): src = up to 4 int32 arrays parallel to ids (token offsets, labels, ...),
    fill = one int per array.  Returns ids_to_rows_batch's five results and the list of planes, int32[R, L] each: a cell that holds an id holds
    that id's element of the array, every other cell the array's fill."""
    ids = np.ascontiguousarray(ids, dtype=np.int32)
    id_off = np.ascontiguousarray(id_off, dtype=np.int64)
    src = [_np_i32(x) for x in src]
    nseq = len(id_off) - 1
    pre = (c_void_p(h), ids.ctypes.data, id_off.ctypes.data, nseq, int(L), _special(cls_id), _special(sep_id), int(pad_id), int(stride),
           int(max_rows_per_seq), int(bool(pad_left)))
    return _rows_host("IdsToRowsPlanesBatch", pre, nseq, L, (np.int32, np.uint8), _plane_tail([src], fill, lambda a: a.ctypes.data))


def ids_to_rows_planes_batch_device(h, d_ids, d_id_off, L, cls_id=None, sep_id=None, pad_id=0, stride=0, max_rows_per_seq=1, pad_left=False,
                                    rows_cap=None, stream=None, src=(), fill=()):
    """Device-resident ids_to_rows_planes_batch: src = int32 tensors on the device of d_ids, parallel to it (the starts / ends of
    text_to_ids_with_offsets_batch_device as they are).  Returns ids_to_rows_batch_device's five results and the list of plane tensors."""
    import torch
    nseq = d_id_off.numel() - 1
    pre = (c_void_p(h), d_ids.data_ptr(), d_ids.numel(), d_id_off.data_ptr(), nseq, int(L), _special(cls_id), _special(sep_id), int(pad_id),
           int(stride), int(max_rows_per_seq), int(bool(pad_left)))
    return _rows_device("IdsToRowsPlanesBatchDevice", pre, nseq, L, (torch.int32, torch.uint8), max_rows_per_seq == 1, rows_cap, d_ids.device, stream,
                        _plane_tail([[_dev_i32(t, d_ids.device, "ids_to_rows_planes_batch_device: src[%d]" % k) for k, t in enumerate(src)]], fill, lambda t: t.data_ptr()))


def rows_span_cells_device(h, starts, ends, row_seq, row_offsets, span_first, span_last, none_cell=0, stream=None):
    """An item's byte span [span_first[q], span_last[q]] (the last byte inclusive) -> the cells of each of its rows whose tokens hold the span's
    two ends (RowsSpanCellsBatchDevice).  starts / ends: int32[R, L] planes of token offsets with a negative fill (ids_to_*_planes_batch_device
    over the tokenizer's offsets); row_seq: int32[R] the item of every row, or None (row r is item r); row_offsets: the int64[nseq+1] row
    offsets of the call that made the planes (its last entry bounds the rows, on the device), or None (every row of the planes; the items are then as many as span_first has entries).
    Returns (start_cell int32[R], end_cell int32[R]); none_cell in both where the span is not inside the row.  Like every batch call it clears
    the handle's status word first: BfLastStatus afterwards is this call's (bit 3: a row whose item is out of range), not the row call's."""
    import torch
    dev = starts.device
    for what, t in (("starts", starts), ("ends", ends), ("row_seq", row_seq)):
        _dev_i32(t, dev, "rows_span_cells_device: " + what)
    if starts.dim() != 2 or ends.shape != starts.shape or (row_seq is not None and row_seq.numel() != starts.shape[0]):
        raise ValueError("rows_span_cells_device: starts and ends are [R, L] planes of one shape, row_seq has R entries")
    if row_offsets is not None and (row_offsets.dtype != torch.int64 or not row_offsets.is_contiguous() or row_offsets.device != dev):
        raise ValueError("rows_span_cells_device: row_offsets must be a contiguous torch.int64 tensor on %s" % dev)
    R, L = starts.shape
    span_first = span_first.to(device=dev, dtype=torch.int32).contiguous(); span_last = span_last.to(device=dev, dtype=torch.int32).contiguous()
    nseq = row_offsets.numel() - 1 if row_offsets is not None else span_first.numel()          # (without row offsets the spans say how many items there are)
    if span_first.numel() != span_last.numel() or span_first.numel() < nseq:
        raise ValueError("rows_span_cells_device: span_first / span_last need one entry per item (%d)" % nseq)
    out = [torch.full((R,), int(none_cell), dtype=torch.int32, device=starts.device) for _ in range(2)]
    s = stream if stream is not None else torch.cuda.current_stream(starts.device).cuda_stream
    r = lib().RowsSpanCellsBatchDevice(c_void_p(h), starts.data_ptr(), ends.data_ptr(), L, R,
                                       None if row_offsets is None else row_offsets.data_ptr() + 8 * nseq, None if row_seq is None else row_seq.data_ptr(),
                                       nseq, span_first.data_ptr(), span_last.data_ptr(), int(none_cell), out[0].data_ptr(), out[1].data_ptr(), c_void_p(s))
    if r != 0:
        raise RuntimeError("RowsSpanCellsBatchDevice failed (%d): %s" % (r, lib().BfLastError().decode("utf-8", "replace")))
    return out[0], out[1]


def encode_batch_device(h, d_text, d_doc_off, L, cls_id, sep_id, pad_id, unk=0, stride=0, max_rows_per_doc=1, pad_left=False, return_offsets=False):
    """Text in HBM -> tensors a model takes, nothing on the host: text_to_ids_batch_device and ids_to_rows_batch_device on one stream.
    Every document is tokenised up to the ids its rows can hold (all of them when max_rows_per_doc is 0).
    Returns (rows int32[R, L], mask uint8[R, L], row_doc int32[R], row_offsets int64[ndocs+1]); with return_offsets also
    (starts int32[R, L], ends int32[R, L]): every token's first and last byte in its document, -1 in cells without a token."""
    body = int(L) - (1 if _special(cls_id) >= 0 else 0) - (1 if _special(sep_id) >= 0 else 0)
    step = body - int(stride)
    if body < 1 or stride < 0 or step < 1 or max_rows_per_doc < 0:
        raise ValueError("encode_batch_device: L leaves no room for ids, or stride / max_rows_per_doc are out of range")
    max_len = min(body + (max_rows_per_doc - 1) * step, 2 ** 31 - 1) if max_rows_per_doc > 0 else 2 ** 31 - 1
    if return_offsets:
        d_ids, d_st, d_en, d_id_off = text_to_ids_with_offsets_batch_device(h, d_text, d_doc_off, max_len, unk)
        rows, mask, seq, _, r_off, (st, en) = ids_to_rows_planes_batch_device(h, d_ids, d_id_off, L, cls_id, sep_id, pad_id, stride, max_rows_per_doc, pad_left,
                                                                               src=[d_st, d_en], fill=[-1, -1])
        return rows, mask, seq, r_off, st, en
    d_ids, d_id_off = text_to_ids_batch_device(h, d_text, d_doc_off, max_len, unk)
    rows, mask, seq, _, r_off = ids_to_rows_batch_device(h, d_ids, d_id_off, L, cls_id, sep_id, pad_id, stride, max_rows_per_doc, pad_left)
    return rows, mask, seq, r_off


def encode_batch(h, docs, L, cls_id, sep_id, pad_id, unk=0, stride=0, max_rows_per_doc=1, pad_left=False):
    """encode_batch_device for a list of str / bytes (or a (uint8 array, int64 offsets) pair): packed, uploaded with torch to the current
    device, encoded there."""
    import torch
    text, off = docs if isinstance(docs, tuple) else pack_docs(docs)
    d_text = torch.from_numpy(np.ascontiguousarray(text, dtype=np.uint8).copy()).cuda()
    d_off = torch.from_numpy(np.ascontiguousarray(off, dtype=np.int64).copy()).cuda()
    return encode_batch_device(h, d_text, d_off, L, cls_id, sep_id, pad_id, unk, stride, max_rows_per_doc, pad_left)


def _pair_args(L, cls_id, sep_id, pad_id, mode, max_a, stride, max_rows_per_pair, pad_left, double_sep):
    return (int(L), _special(cls_id), _special(sep_id), int(pad_id), int(mode), int(max_a), int(stride), int(max_rows_per_pair),
            (1 if pad_left else 0) | (2 if double_sep else 0))


def ids_to_pair_rows_batch(h, ids_a, off_a, ids_b, off_b, L, cls_id=None, sep_id=None, pad_id=0, mode=1, max_a=0, stride=0, max_rows_per_pair=1,
                           pad_left=False, double_sep=False):
    """additive: pairs of ragged ids (two int32 arrays + two int64 offsets[nseq+1]) -> [cls] A [sep] B [sep] rows with type ids
    (IdsToPairRowsBatch).  mode 1: one row per pair, ids dropped from the end of the longer side until both fit (max_a, stride and
    max_rows_per_pair stay at their defaults).  mode 0: the first max_a ids of A in every row, B cut into windows that share `stride` ids
    (max_rows_per_pair: 1 = truncate B, 0 = every window).  double_sep: two separators between A and B.  Returns (rows int32[R, L],
    mask uint8[R, L], type uint8[R, L], row_pair int32[R], row_first_b int32[R], row_offsets int64[nseq+1]): the rows of pair q are
    [row_offsets[q], row_offsets[q+1]), row_first_b is the index within B of a row's first B id."""
    ids_a = np.ascontiguousarray(ids_a, dtype=np.int32); off_a = np.ascontiguousarray(off_a, dtype=np.int64)
    ids_b = np.ascontiguousarray(ids_b, dtype=np.int32); off_b = np.ascontiguousarray(off_b, dtype=np.int64)
    nseq = len(off_a) - 1
    if len(off_b) != nseq + 1:
        raise ValueError("ids_to_pair_rows_batch: off_a and off_b name different numbers of sequences")
    pre = (c_void_p(h), ids_a.ctypes.data, off_a.ctypes.data, ids_b.ctypes.data, off_b.ctypes.data, nseq) + _pair_args(
        L, cls_id, sep_id, pad_id, mode, max_a, stride, max_rows_per_pair, pad_left, double_sep)
    return _rows_host("IdsToPairRowsBatch", pre, nseq, L, (np.int32, np.uint8, np.uint8))


def ids_to_pair_rows_batch_device(h, d_ids_a, d_off_a, d_ids_b, d_off_b, L, cls_id=None, sep_id=None, pad_id=0, mode=1, max_a=0, stride=0,
                                  max_rows_per_pair=1, pad_left=False, double_sep=False, rows_cap=None, stream=None):
    """Device-resident ids_to_pair_rows_batch: torch int32 ids + int64 offsets of both sides on one GPU (the results of two
    text_to_ids_batch_device calls as they are; the same tensor may serve both sides) -> the same six results as tensors on that device,
    enqueued on torch's current stream (or `stream`).  rows_cap None: nseq rows when one row per pair is certain (mode 1, or
    max_rows_per_pair 1: nothing is read back); otherwise a size query whose total is read back (one synchronisation).  With a rows_cap of
    the caller's the tensors have rows_cap rows, row_offsets[-1] of them valid; rows beyond it are dropped (BfLastStatus bit 0)."""
    import torch
    nseq = d_off_a.numel() - 1
    if d_off_b.numel() != nseq + 1:
        raise ValueError("ids_to_pair_rows_batch_device: d_off_a and d_off_b name different numbers of sequences")
    pre = (c_void_p(h), d_ids_a.data_ptr(), d_ids_a.numel(), d_off_a.data_ptr(), d_ids_b.data_ptr(), d_ids_b.numel(), d_off_b.data_ptr(), nseq) + _pair_args(
        L, cls_id, sep_id, pad_id, mode, max_a, stride, max_rows_per_pair, pad_left, double_sep)
    return _rows_device("IdsToPairRowsBatchDevice", pre, nseq, L, (torch.int32, torch.uint8, torch.uint8), mode == 1 or max_rows_per_pair == 1, rows_cap,
                        d_ids_a.device, stream)


def _pair_sides(src_a, src_b, n):
    return [list(src_a) if src_a is not None else [None] * n, list(src_b) if src_b is not None else [None] * n]


def ids_to_pair_rows_planes_batch(h, ids_a, off_a, ids_b, off_b, L, cls_id=None, sep_id=None, pad_id=0, mode=1, max_a=0, stride=0, max_rows_per_pair=1,
                                  pad_left=False, double_sep=False, src_a=None, src_b=None, fill=()):
    """ids_to_pair_rows_batch with companion planes (IdsToPairRowsPlanesBatch): src_a / src_b = lists of int32 arrays parallel to ids_a / ids_b,
    one entry per fill value; a list that is None, or an entry that is, leaves that side's cells at the fill.  Returns ids_to_pair_rows_batch's
    six results and the list of planes, int32[R, L] each."""
    ids_a = np.ascontiguousarray(ids_a, dtype=np.int32); off_a = np.ascontiguousarray(off_a, dtype=np.int64)
    ids_b = np.ascontiguousarray(ids_b, dtype=np.int32); off_b = np.ascontiguousarray(off_b, dtype=np.int64)
    nseq = len(off_a) - 1
    if len(off_b) != nseq + 1:
        raise ValueError("ids_to_pair_rows_planes_batch: off_a and off_b name different numbers of sequences")
    sides = [[_np_i32(x) for x in side] for side in _pair_sides(src_a, src_b, len(fill))]
    pre = (c_void_p(h), ids_a.ctypes.data, off_a.ctypes.data, ids_b.ctypes.data, off_b.ctypes.data, nseq) + _pair_args(
        L, cls_id, sep_id, pad_id, mode, max_a, stride, max_rows_per_pair, pad_left, double_sep)
    return _rows_host("IdsToPairRowsPlanesBatch", pre, nseq, L, (np.int32, np.uint8, np.uint8), _plane_tail(sides, fill, lambda a: a.ctypes.data))


def ids_to_pair_rows_planes_batch_device(h, d_ids_a, d_off_a, d_ids_b, d_off_b, L, cls_id=None, sep_id=None, pad_id=0, mode=1, max_a=0, stride=0,
                                         max_rows_per_pair=1, pad_left=False, double_sep=False, rows_cap=None, stream=None, src_a=None, src_b=None, fill=()):
    """Device-resident ids_to_pair_rows_planes_batch: src_a / src_b = lists of int32 tensors parallel to d_ids_a / d_ids_b (None entries and
    None lists allowed).  Returns ids_to_pair_rows_batch_device's six results and the list of plane tensors."""
    import torch
    nseq = d_off_a.numel() - 1
    if d_off_b.numel() != nseq + 1:
        raise ValueError("ids_to_pair_rows_planes_batch_device: d_off_a and d_off_b name different numbers of sequences")
    pre = (c_void_p(h), d_ids_a.data_ptr(), d_ids_a.numel(), d_off_a.data_ptr(), d_ids_b.data_ptr(), d_ids_b.numel(), d_off_b.data_ptr(), nseq) + _pair_args(
        L, cls_id, sep_id, pad_id, mode, max_a, stride, max_rows_per_pair, pad_left, double_sep)
    return _rows_device("IdsToPairRowsPlanesBatchDevice", pre, nseq, L, (torch.int32, torch.uint8, torch.uint8), mode == 1 or max_rows_per_pair == 1, rows_cap,
                        d_ids_a.device, stream, _plane_tail([[_dev_i32(t, d_ids_a.device, "ids_to_pair_rows_planes_batch_device: src_%s[%d]" % (ab, k))
                                                              for k, t in enumerate(side)] for ab, side in zip("ab", _pair_sides(src_a, src_b, len(fill)))],
                                                            fill, lambda t: t.data_ptr()))


def encode_pairs_batch_device(h, d_text_a, d_off_a, d_text_b, d_off_b, L, cls_id, sep_id, pad_id, unk=0, mode=1, max_a=0, stride=0, max_rows_per_pair=1,
                              pad_left=False, double_sep=False, return_offsets=False, offsets_a=False):
    """Two texts in HBM -> the tensors a pair model takes, nothing on the host: two text_to_ids_batch_device calls and
    ids_to_pair_rows_batch_device on one stream.  Each side is tokenised up to the ids its rows can hold: T = L - specials for both in mode 1
    (cutting both to T first does not change what longest-first keeps); in mode 0 max_a for A and T + (max_rows_per_pair - 1) * (T - stride)
    for B (all of B when max_rows_per_pair is 0).
    Returns (rows int32[R, L], mask uint8[R, L], type uint8[R, L], row_pair int32[R], row_first_b int32[R], row_offsets int64[npairs+1]); with
    return_offsets also (starts int32[R, L], ends int32[R, L]): first and last byte of every token of B in its text (with offsets_a, of A in
    its own text too), -1 in every other cell."""
    nsep = 0 if _special(sep_id) < 0 else 3 if double_sep else 2
    T = int(L) - (1 if _special(cls_id) >= 0 else 0) - nsep
    if T < 1 or mode not in (0, 1) or (mode == 0 and not (0 <= max_a <= T - 1 and 0 <= stride < T - max_a and max_rows_per_pair >= 0)):
        raise ValueError("encode_pairs_batch_device: L leaves no room for ids, or mode / max_a / stride / max_rows_per_pair are out of range")
    if mode == 1:
        len_a = len_b = T
    else:
        len_a = int(max_a)
        len_b = min(T + (max_rows_per_pair - 1) * (T - int(stride)), 2 ** 31 - 1) if max_rows_per_pair > 0 else 2 ** 31 - 1
    if return_offsets:
        src_a = None
        if offsets_a:
            d_ids_a, d_st_a, d_en_a, d_idoff_a = text_to_ids_with_offsets_batch_device(h, d_text_a, d_off_a, len_a, unk)
            src_a = [d_st_a, d_en_a]
        else:
            d_ids_a, d_idoff_a = text_to_ids_batch_device(h, d_text_a, d_off_a, len_a, unk)
        d_ids_b, d_st_b, d_en_b, d_idoff_b = text_to_ids_with_offsets_batch_device(h, d_text_b, d_off_b, len_b, unk)
        *base, (st, en) = ids_to_pair_rows_planes_batch_device(h, d_ids_a, d_idoff_a, d_ids_b, d_idoff_b, L, cls_id, sep_id, pad_id, mode, max_a, stride,
                                                              max_rows_per_pair, pad_left, double_sep, src_a=src_a, src_b=[d_st_b, d_en_b], fill=[-1, -1])
        return (*base, st, en)
    d_ids_a, d_idoff_a = text_to_ids_batch_device(h, d_text_a, d_off_a, len_a, unk)
    d_ids_b, d_idoff_b = text_to_ids_batch_device(h, d_text_b, d_off_b, len_b, unk)
    return ids_to_pair_rows_batch_device(h, d_ids_a, d_idoff_a, d_ids_b, d_idoff_b, L, cls_id, sep_id, pad_id, mode, max_a, stride, max_rows_per_pair,
                                         pad_left, double_sep)


def encode_qa_batch_device(h, d_text_q, d_off_q, d_text_c, d_off_c, L, cls_id, sep_id, pad_id, max_q, stride, unk=0, double_sep=False, d_ans_first=None,
                           d_ans_last=None):
    """Questions and contexts in HBM -> extractive-QA inputs, one stream end to end: [cls] question [sep] context window [sep] rows (mode 0,
    the first max_q question ids in every row, every window of the context, `stride` ids shared by neighbours) with the context's byte
    offsets as planes.  Returns (rows, mask, type, row_pair, row_first_b, row_offsets, starts, ends) -- starts / ends int32[R, L]: first and
    last byte of every context token in its context, -1 elsewhere -- and, with d_ans_first / d_ans_last (int32[npairs]: first and last byte,
    inclusive, of each answer in its context; negative = none), also (start_cell, end_cell) int32[R]: the token cells of the answer in every
    row, the [cls] cell (0) in both where the answer is not inside the row's window.  The only read-back is the size query of
    ids_to_pair_rows_batch_device.  BfLastStatus afterwards is that of the LAST call on the handle alone, as always: with answers that is the span
    call, which cleared what the tokenizer and row calls reported (ids or rows dropped, bad ranges); a caller who needs those runs
    encode_pairs_batch_device(..., return_offsets=True) and rows_span_cells_device itself and reads the status between them."""
    out = encode_pairs_batch_device(h, d_text_q, d_off_q, d_text_c, d_off_c, L, cls_id, sep_id, pad_id, unk, 0, max_q, stride, 0, False, double_sep,
                                    return_offsets=True)
    if d_ans_first is None or d_ans_last is None:
        return out
    return (*out, *rows_span_cells_device(h, out[6], out[7], out[3], out[5], d_ans_first, d_ans_last, 0))


def encode_pairs_batch(h, docs_a, docs_b, L, cls_id, sep_id, pad_id, unk=0, mode=1, max_a=0, stride=0, max_rows_per_pair=1, pad_left=False, double_sep=False):
    """encode_pairs_batch_device for two lists of str / bytes (or two (uint8 array, int64 offsets) pairs): packed, uploaded with torch to the
    current device, encoded there."""
    import torch
    d = []
    for docs in (docs_a, docs_b):
        text, off = docs if isinstance(docs, tuple) else pack_docs(docs)
        d.append(torch.from_numpy(np.ascontiguousarray(text, dtype=np.uint8).copy()).cuda())
        d.append(torch.from_numpy(np.ascontiguousarray(off, dtype=np.int64).copy()).cuda())
    return encode_pairs_batch_device(h, d[0], d[1], d[2], d[3], L, cls_id, sep_id, pad_id, unk, mode, max_a, stride, max_rows_per_pair, pad_left, double_sep)


def ids_to_packed_rows_batch(h, ids, id_off, L, cls_id=None, sep_id=None, pad_id=0):
    """additive: ragged ids (int32 array + int64 offsets[nseq+1]) -> PACKED model inputs (IdsToPackedRowsBatch): several sequences share a
    row, filled greedily and in order; a sequence longer than a row is truncated, none is split.  cls_id / sep_id None = no such special.
    Returns (rows int32[R, L], seg int32[R, L], pos int32[R, L], row_first_seq int32[R + 1], seq_row int32[nseq], seq_col int32[nseq]):
    seg numbers the sequences of a row from 1 (0 = padding), pos restarts at every sequence, row r holds the sequences
    [row_first_seq[r], row_first_seq[r + 1]), and sequence q begins at cell seq_col[q] of row seq_row[q]."""
    return _packed_host("IdsToPackedRowsBatch", h, ids, id_off, L, cls_id, sep_id, pad_id)


def _packed_host(name, h, ids, id_off, L, cls_id, sep_id, pad_id, extra=None):
    """the host forms of the packed call: the size query, then every output.  extra = (nplanes, tail) of _plane_tail: the ...Planes call, whose
    int32 [R, L] planes are appended to the result as a list"""
    ids = np.ascontiguousarray(ids, dtype=np.int32)
    id_off = np.ascontiguousarray(id_off, dtype=np.int64)
    nseq = len(id_off) - 1
    fn = getattr(lib(), name)
    nextra, tail = extra if extra else (0, lambda outs: ())
    pre = (c_void_p(h), ids.ctypes.data, id_off.ctypes.data, nseq, int(L), _special(cls_id), _special(sep_id), int(pad_id), 0)
    seq_row = np.empty(nseq, dtype=np.int32)
    seq_col = np.empty(nseq, dtype=np.int32)
    n = fn(*pre, None, None, None, None, 0, seq_row.ctypes.data, seq_col.ctypes.data, *tail(None))
    if n < 0:
        raise RuntimeError("%s failed: %d (%s)" % (name, n, lib().BfLastError().decode("utf-8", "replace")))
    planes = [np.empty((n, L), dtype=np.int32) for _ in range(3)]
    more = [np.empty((n, L), dtype=np.int32) for _ in range(nextra)]
    first = np.empty(n + 1, dtype=np.int32)
    r = fn(*pre, *[p.ctypes.data for p in planes], first.ctypes.data, n, seq_row.ctypes.data, seq_col.ctypes.data, *tail(more))
    if r != n:
        raise RuntimeError("%s failed: %d (%s)" % (name, r, lib().BfLastError().decode("utf-8", "replace")))
    return (*planes, first, seq_row, seq_col, more) if extra else (*planes, first, seq_row, seq_col)


def ids_to_packed_rows_planes_batch(h, ids, id_off, L, cls_id=None, sep_id=None, pad_id=0, src=(), fill=()):
    """ids_to_packed_rows_batch with companion planes (IdsToPackedRowsPlanesBatch): src = up to 4 int32 arrays parallel to ids (token offsets,
    labels, ...), fill = one int per array.  Returns ids_to_packed_rows_batch's six results and the list of planes, int32[R, L] each: a cell
    that holds an id holds that id's element of the array, every other cell (cls_id, sep_id, padding) the array's fill."""
    src = [_np_i32(x) for x in src]
    return _packed_host("IdsToPackedRowsPlanesBatch", h, ids, id_off, L, cls_id, sep_id, pad_id, _plane_tail([src], fill, lambda a: a.ctypes.data))


def ids_to_packed_rows_batch_device(h, d_ids, d_id_off, L, cls_id=None, sep_id=None, pad_id=0, rows_cap=None, stream=None, planes=None, fill=None):
    """Device-resident ids_to_packed_rows_batch: torch int32 ids + int64 offsets on one GPU (text_to_ids_batch_device's results as they are)
    -> (rows, seg, pos, row_first_seq, seq_row, seq_col, nrows) as tensors on that device, enqueued on torch's current stream (or `stream`);
    nrows is int64[1], the row count R.  rows_cap None: a size query whose R is read back (one synchronisation), the tensors have R rows.
    With a rows_cap of the caller's nothing is read back: the planes have rows_cap rows and row_first_seq rows_cap + 1 entries, of which
    min(R, rows_cap) rows and one entry more are written; rows beyond it are dropped (BfLastStatus bit 0).
    planes: a list of up to 4 int32 tensors on that device, parallel to d_ids (the starts / ends of text_to_ids_with_offsets_batch_device as
    they are, per-token labels, ...), fill: one int per tensor (IdsToPackedRowsPlanesBatchDevice).  The gathered planes, int32[rows, L] each,
    are appended behind nrows: a cell that holds an id holds that id's element, every other cell the fill."""
    import torch
    dev = d_ids.device
    nseq = d_id_off.numel() - 1
    if planes is None and fill:
        raise ValueError("ids_to_packed_rows_batch_device: fill without planes")
    nextra, tail = 0, lambda outs: ()
    if planes is not None:
        nextra, tail = _plane_tail([[_dev_i32(t, dev, "ids_to_packed_rows_batch_device: planes[%d]" % k) for k, t in enumerate(planes)]],
                                   () if fill is None else fill, lambda t: t.data_ptr())
    name = "IdsToPackedRowsBatchDevice" if planes is None else "IdsToPackedRowsPlanesBatchDevice"
    fn = getattr(lib(), name)
    s = c_void_p(stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream)
    pre = (c_void_p(h), d_ids.data_ptr(), d_ids.numel(), d_id_off.data_ptr(), nseq, int(L), _special(cls_id), _special(sep_id), int(pad_id), 0)
    nrows = torch.empty(1, dtype=torch.int64, device=dev)

    def call(outs, cap, seq, more=None):
        r = fn(*pre, *outs, cap, *seq, nrows.data_ptr(), *tail(more), s)
        if r != 0:
            raise RuntimeError("%s failed (%d): %s" % (name, r, lib().BfLastError().decode("utf-8", "replace")))
    if rows_cap is None:
        call([None] * 4, 0, [None] * 2)
        if stream is not None:
            torch.cuda.synchronize(dev)                   # (a raw stream handle: nothing finer to wait on)
        rows_cap = int(nrows.item())
    base = [torch.empty((rows_cap, L), dtype=torch.int32, device=dev) for _ in range(3)]
    more = [torch.empty((rows_cap, L), dtype=torch.int32, device=dev) for _ in range(nextra)]
    first = torch.empty(rows_cap + 1, dtype=torch.int32, device=dev)
    seq = [torch.empty(nseq, dtype=torch.int32, device=dev) for _ in range(2)]
    call([t.data_ptr() for t in base] + [first.data_ptr()], rows_cap, [t.data_ptr() for t in seq], more)
    return (*base, first, *seq, nrows, *more)


def encode_packed_batch_device(h, d_text, d_doc_off, L, cls_id, sep_id, pad_id, unk=0, rows_cap=None, return_offsets=False):
    """Text in HBM -> packed tensors a model takes, nothing on the host: text_to_ids_batch_device (every document tokenised up to the ids
    a row can hold) and ids_to_packed_rows_batch_device on one stream.  Returns what ids_to_packed_rows_batch_device returns; with a
    rows_cap of the caller's nothing is read back.  With return_offsets also (starts int32[R, L], ends int32[R, L]) behind nrows: every
    token's first and last byte in its document, -1 in cells without a token."""
    body = int(L) - (1 if _special(cls_id) >= 0 else 0) - (1 if _special(sep_id) >= 0 else 0)
    if body < 1:
        raise ValueError("encode_packed_batch_device: L leaves no room for ids")
    if return_offsets:
        d_ids, d_st, d_en, d_id_off = text_to_ids_with_offsets_batch_device(h, d_text, d_doc_off, body, unk)
        return ids_to_packed_rows_batch_device(h, d_ids, d_id_off, L, cls_id, sep_id, pad_id, rows_cap, planes=[d_st, d_en], fill=[-1, -1])
    d_ids, d_id_off = text_to_ids_batch_device(h, d_text, d_doc_off, body, unk)
    return ids_to_packed_rows_batch_device(h, d_ids, d_id_off, L, cls_id, sep_id, pad_id, rows_cap)


def encode_packed_batch(h, docs, L, cls_id, sep_id, pad_id, unk=0, rows_cap=None):
    """encode_packed_batch_device for a list of str / bytes (or a (uint8 array, int64 offsets) pair): packed into one buffer, uploaded with
    torch to the current device, encoded there."""
    import torch
    text, off = docs if isinstance(docs, tuple) else pack_docs(docs)
    d_text = torch.from_numpy(np.ascontiguousarray(text, dtype=np.uint8).copy()).cuda()
    d_off = torch.from_numpy(np.ascontiguousarray(off, dtype=np.int64).copy()).cuda()
    return encode_packed_batch_device(h, d_text, d_off, L, cls_id, sep_id, pad_id, unk, rows_cap)


def _stream_flags(drop_last, pos_from_row, labels_within_doc):
    return (1 if drop_last else 0) | (2 if pos_from_row else 0) | (4 if labels_within_doc else 0)


def ids_to_stream_rows_batch(h, ids, id_off, L, bos_id=None, eos_id=None, pad_id=0, ignore_label=-100, drop_last=False, pos_from_row=False,
                             labels_within_doc=False):
    """additive: ragged ids (int32 array + int64 offsets[nseq+1]) -> STREAM rows for causal-LM training (IdsToStreamRowsBatch): every sequence
    closed by its specials, all of them laid end to end, the stream cut into rows of exactly L cells; a sequence runs over a row's edge into the
    next row, nothing is truncated and nothing is padded but the tail.  bos_id / eos_id None = no such special.
    Returns (rows, seg, pos, labels int32[R, L], row_first_seq, row_first_pos int32[R], seq_row, seq_col int32[nseq]): labels are the next
    element of the stream (ignore_label behind the last one, and, with labels_within_doc, where the next element belongs to another sequence);
    seg numbers the sequences of a row from 1 (0 = padding); pos is the place in the sequence, continuing across rows (pos_from_row: counted
    from the row's edge for a sequence that continues from the row before); row r begins at place row_first_pos[r] of sequence
    row_first_seq[r]; sequence q begins at cell seq_col[q] of row seq_row[q].  drop_last drops the last row when it is incomplete."""
    ids = np.ascontiguousarray(ids, dtype=np.int32)
    id_off = np.ascontiguousarray(id_off, dtype=np.int64)
    nseq = len(id_off) - 1
    fn = lib().IdsToStreamRowsBatch
    pre = (c_void_p(h), ids.ctypes.data, id_off.ctypes.data, nseq, int(L), _special(bos_id), _special(eos_id), int(pad_id), int(ignore_label),
           _stream_flags(drop_last, pos_from_row, labels_within_doc))
    seq = [np.empty(nseq, dtype=np.int32) for _ in range(2)]
    n = fn(*pre, *[None] * 6, 0, *[a.ctypes.data for a in seq])
    if n < 0:
        raise RuntimeError("IdsToStreamRowsBatch failed: %d (%s)" % (n, lib().BfLastError().decode("utf-8", "replace")))
    outs = [np.empty((n, L), dtype=np.int32) for _ in range(4)] + [np.empty(n, dtype=np.int32) for _ in range(2)]
    r = fn(*pre, *[a.ctypes.data for a in outs], n, *[a.ctypes.data for a in seq])
    if r != n:
        raise RuntimeError("IdsToStreamRowsBatch failed: %d (%s)" % (r, lib().BfLastError().decode("utf-8", "replace")))
    return (*outs, *seq)


def ids_to_stream_rows_batch_device(h, d_ids, d_id_off, L, bos_id=None, eos_id=None, pad_id=0, ignore_label=-100, drop_last=False, pos_from_row=False,
                                    labels_within_doc=False, rows_cap=None, stream=None):
    """Device-resident ids_to_stream_rows_batch: torch int32 ids + int64 offsets on one GPU (text_to_ids_batch_device's results as they are)
    -> (rows, seg, pos, labels, row_first_seq, row_first_pos, seq_row, seq_col, nrows) as tensors on that device, enqueued on torch's current
    stream (or `stream`); nrows is int64[2] = {R, T}: the row count and the length of the stream.  Nothing is read back: rows_cap None uses the
    bound the host knows, ceil((d_ids.numel() + specials * nseq) / L).  The row outputs have rows_cap rows, of which min(R, rows_cap) are
    written; rows beyond rows_cap are dropped (BfLastStatus bit 0)."""
    import torch
    dev = d_ids.device
    nseq = d_id_off.numel() - 1
    L = int(L)
    if rows_cap is None:
        specials = (1 if _special(bos_id) >= 0 else 0) + (1 if _special(eos_id) >= 0 else 0)
        rows_cap = -(-(d_ids.numel() + specials * nseq) // L) if L > 0 else 0
    s = c_void_p(stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream)
    outs = [torch.empty((rows_cap, L), dtype=torch.int32, device=dev) for _ in range(4)] + [torch.empty(rows_cap, dtype=torch.int32, device=dev) for _ in range(2)]
    seq = [torch.empty(nseq, dtype=torch.int32, device=dev) for _ in range(2)]
    nrows = torch.empty(2, dtype=torch.int64, device=dev)
    r = lib().IdsToStreamRowsBatchDevice(c_void_p(h), d_ids.data_ptr(), d_ids.numel(), d_id_off.data_ptr(), nseq, L, _special(bos_id), _special(eos_id), int(pad_id),
                                         int(ignore_label), _stream_flags(drop_last, pos_from_row, labels_within_doc), *[t.data_ptr() for t in outs], rows_cap,
                                         *[t.data_ptr() for t in seq], nrows.data_ptr(), s)
    if r != 0:
        raise RuntimeError("IdsToStreamRowsBatchDevice failed (%d): %s" % (r, lib().BfLastError().decode("utf-8", "replace")))
    return (*outs, *seq, nrows)


def encode_clm_batch_device(h, d_text, d_doc_off, L, bos_id, eos_id, pad_id, unk=0, ignore_label=-100, drop_last=False, pos_from_row=False,
                            labels_within_doc=False, rows_cap=None, max_ids_per_doc=0x7fffffff):
    """Text in HBM -> the tensors causal-LM training takes, nothing on the host and nothing read back: text_to_ids_batch_device (every
    document tokenised, up to max_ids_per_doc ids) and ids_to_stream_rows_batch_device on one stream.  Returns a dict: input_ids, seg, pos,
    labels (int32[rows_cap, L]), row_first_seq, row_first_pos (int32[rows_cap]), seq_row, seq_col (int32[ndocs]) and nrows (int64[2] = {R, T});
    rows_cap None = the bound the host knows from the size of the tokenizer's id buffer."""
    d_ids, d_id_off = text_to_ids_batch_device(h, d_text, d_doc_off, int(max_ids_per_doc), unk)
    got = ids_to_stream_rows_batch_device(h, d_ids, d_id_off, L, bos_id, eos_id, pad_id, ignore_label, drop_last, pos_from_row, labels_within_doc, rows_cap)
    return dict(zip(("input_ids", "seg", "pos", "labels", "row_first_seq", "row_first_pos", "seq_row", "seq_col", "nrows"), got))


def encode_clm_batch(h, docs, L, bos_id, eos_id, pad_id, unk=0, ignore_label=-100, drop_last=False, pos_from_row=False, labels_within_doc=False,
                     rows_cap=None, max_ids_per_doc=0x7fffffff):
    """encode_clm_batch_device for a list of str / bytes (or a (uint8 array, int64 offsets) pair): packed into one buffer, uploaded with
    torch to the current device, encoded there."""
    import torch
    text, off = docs if isinstance(docs, tuple) else pack_docs(docs)
    d_text = torch.from_numpy(np.ascontiguousarray(text, dtype=np.uint8).copy()).cuda()
    d_off = torch.from_numpy(np.ascontiguousarray(off, dtype=np.int64).copy()).cuda()
    return encode_clm_batch_device(h, d_text, d_off, L, bos_id, eos_id, pad_id, unk, ignore_label, drop_last, pos_from_row, labels_within_doc, rows_cap, max_ids_per_doc)


def rows_mlm_mask_device(h, rows, *, mask=None, seg=None, starts=None, ends=None, nrows=None, special_ids=(), select_prob=0.15, mask_prob=0.8, random_prob=0.1,
                         mask_id, rand_range, ignore_label=-100, seed, epoch=0, inplace=False, stream=None, max_predictions=0):
    """Masked-language-model masking of rows that are on the device (RowsMlmMaskBatchDevice): -> (ids int32[R, L], labels int32[R, L]).
    max_predictions = P > 0 (RowsMlmPredictionsBatchDevice): at most P predictions per row -- the selected units in the order of a key they
    draw, as long as they fit, whole words whole -- and -> (ids, labels, pred_cells int32[R, P], pred_labels int32[R, P], pred_count int32[R]):
    the predicted cells of a row in cell order, their original ids, and how many there are; behind them, and in rows at or past nrows,
    cell 0 and ignore_label.  hidden.gather(1, pred_cells.long()[..., None].expand(-1, -1, H)) are the positions to project.  L <= 4096 then.
    rows: int32[R, L] from any of the row calls; mask: uint8[R, L] or None; seg: int32[R, L] (the packed call's segment plane) or None; a cell
    outside the mask, in segment 0 or holding one of special_ids (at most 8) is never masked.  starts / ends: int32[R, L] planes of token
    offsets with a negative fill (both or neither): with them a run of byte-adjacent tokens is selected as a whole (whole-word masking for
    WordPiece models), without them every token on its own.  nrows: an int64 tensor of one element on the device that bounds the rows (a view
    such as row_offsets[-1:]), or None (every row).  A selected cell gets labels = its id and ids = mask_id with mask_prob, a random id
    of rand_range = (lo, hi), hi exclusive, with random_prob, its own id otherwise; every other cell keeps its id and gets ignore_label.
    The result is a function of (seed, epoch, row, cell) and the row alone: the same call gives the same result, another epoch another one.
    inplace: ids is `rows` itself, overwritten.  Rows at or past nrows of a fresh ids tensor are copies of `rows`, of labels ignore_label.
    Like every batch call it clears the handle's status word first."""
    import torch
    dev = rows.device
    for what, t in (("rows", rows), ("seg", seg), ("starts", starts), ("ends", ends)):
        _dev_i32(t, dev, "rows_mlm_mask_device: " + what)
    if rows.dim() != 2 or any(t is not None and t.shape != rows.shape for t in (mask, seg, starts, ends)):
        raise ValueError("rows_mlm_mask_device: rows is an [R, L] plane; mask, seg, starts and ends have its shape")
    if mask is not None and (not isinstance(mask, torch.Tensor) or mask.dtype != torch.uint8 or not mask.is_contiguous() or mask.device != dev):
        raise ValueError("rows_mlm_mask_device: mask must be a contiguous torch.uint8 tensor on %s" % dev)
    if (starts is None) != (ends is None):
        raise ValueError("rows_mlm_mask_device: starts and ends come together")
    if nrows is not None and (not isinstance(nrows, torch.Tensor) or nrows.dtype != torch.int64 or nrows.numel() != 1 or nrows.device != dev):
        raise ValueError("rows_mlm_mask_device: nrows must be a torch.int64 tensor of one element on %s" % dev)
    special_ids = [int(x) for x in special_ids]
    if len(special_ids) > 8:
        raise ValueError("rows_mlm_mask_device: at most 8 special ids")
    R, L = rows.shape
    if isinstance(max_predictions, bool) or not isinstance(max_predictions, (int, np.integer)) or max_predictions < 0:
        raise ValueError("rows_mlm_mask_device: max_predictions is an integer >= 0")
    P = int(max_predictions)
    if P > 0 and (L > 4096 or P > 1 << 20):
        raise ValueError("rows_mlm_mask_device: max_predictions needs rows of at most 4096 cells and is at most 1 << 20")
    ids = rows if inplace else rows.clone()
    labels = torch.full((R, L), int(ignore_label), dtype=torch.int32, device=dev)
    s = stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream
    c_special = (c_int32 * max(len(special_ids), 1))(*special_ids)

    def addr(t):
        return None if t is None else t.data_ptr()
    if P > 0:
        cells = torch.zeros((R, P), dtype=torch.int32, device=dev)
        plabels = torch.full((R, P), int(ignore_label), dtype=torch.int32, device=dev)
        count = torch.zeros((R,), dtype=torch.int32, device=dev)
        r = lib().RowsMlmPredictionsBatchDevice(c_void_p(h), rows.data_ptr(), L, R, addr(nrows), addr(mask), addr(seg), addr(starts), addr(ends), len(special_ids),
                                                c_special, float(select_prob), float(mask_prob), float(random_prob), int(mask_id), int(rand_range[0]),
                                                int(rand_range[1]), int(ignore_label), int(seed) & 0xFFFFFFFFFFFFFFFF, int(epoch) & 0xFFFFFFFF, ids.data_ptr(),
                                                labels.data_ptr(), P, cells.data_ptr(), plabels.data_ptr(), count.data_ptr(), c_void_p(s))
        if r != 0:
            raise RuntimeError("RowsMlmPredictionsBatchDevice failed (%d): %s" % (r, lib().BfLastError().decode("utf-8", "replace")))
        return ids, labels, cells, plabels, count
    r = lib().RowsMlmMaskBatchDevice(c_void_p(h), rows.data_ptr(), L, R, addr(nrows), addr(mask), addr(seg), addr(starts), addr(ends), len(special_ids), c_special,
                                     float(select_prob), float(mask_prob), float(random_prob), int(mask_id), int(rand_range[0]), int(rand_range[1]), int(ignore_label),
                                     int(seed) & 0xFFFFFFFFFFFFFFFF, int(epoch) & 0xFFFFFFFF, ids.data_ptr(), labels.data_ptr(), c_void_p(s))
    if r != 0:
        raise RuntimeError("RowsMlmMaskBatchDevice failed (%d): %s" % (r, lib().BfLastError().decode("utf-8", "replace")))
    return ids, labels


def encode_mlm_batch_device(h, d_text, d_doc_off, L, cls_id, sep_id, pad_id, mask_id, rand_range, seed, epoch=0, whole_word=False, packed=False, unk=0,
                            special_ids=None, select_prob=0.15, mask_prob=0.8, random_prob=0.1, ignore_label=-100, rows_cap=None, max_predictions=0):
    """Text in HBM -> the tensors of a masked-language-model step, nothing on the host: encode_batch_device (with return_offsets=whole_word)
    or, with packed=True, encode_packed_batch_device, and rows_mlm_mask_device on one stream.  Returns the base call's tuple with the masked
    input ids in place of its rows and `labels` (int32[R, L], ignore_label where nothing is predicted) appended:
    (ids, mask, row_doc, row_offsets[, starts, ends], labels), or packed (ids, seg, pos, row_first_seq, seq_row, seq_col, nrows, labels).
    special_ids None: the cls_id, sep_id and pad_id there are.  Packed rows mask inside the segment plane; this function gives them no offset
    planes, so packed=True with whole_word=True raises ValueError: whole-word masking over packed rows is encode_packed_mlm_batch_device.
    rows_cap is the packed call's (None: its one read-back).  max_predictions = P > 0
    caps the predictions of a row and appends (pred_cells int32[R, P], pred_labels int32[R, P], pred_count int32[R]) behind labels, in all
    three forms (rows_mlm_mask_device)."""
    if packed and whole_word:
        raise ValueError("encode_mlm_batch_device: packed rows have no offset planes, so no whole-word masking")
    if special_ids is None:
        special_ids = [i for i in (_special(cls_id), _special(sep_id), _special(pad_id)) if i >= 0]
    kw = dict(special_ids=special_ids, select_prob=select_prob, mask_prob=mask_prob, random_prob=random_prob, mask_id=mask_id, rand_range=rand_range,
              ignore_label=ignore_label, seed=seed, epoch=epoch, inplace=True, max_predictions=max_predictions)
    if packed:
        out = encode_packed_batch_device(h, d_text, d_doc_off, L, cls_id, sep_id, pad_id, unk, rows_cap)
        ids, *tail = rows_mlm_mask_device(h, out[0], seg=out[1], nrows=out[6], **kw)
        return (ids, *out[1:], *tail)
    out = encode_batch_device(h, d_text, d_doc_off, L, cls_id, sep_id, pad_id, unk, return_offsets=whole_word)
    ids, *tail = rows_mlm_mask_device(h, out[0], mask=out[1], starts=out[4] if whole_word else None, ends=out[5] if whole_word else None, nrows=out[3][-1:], **kw)
    return (ids, *out[1:], *tail)


def encode_packed_mlm_batch_device(h, d_text, d_doc_off, L, cls_id, sep_id, pad_id, mask_id, rand_range, seed, epoch=0, whole_word=True, unk=0,
                                   special_ids=None, select_prob=0.15, mask_prob=0.8, random_prob=0.1, ignore_label=-100, rows_cap=None, max_predictions=0):
    """Text in HBM -> the packed tensors of a masked-language-model step with whole-word masking, nothing on the host: the tokenizer with
    offsets, the packed call with the offsets as companion planes (encode_packed_batch_device(..., return_offsets=True)) and
    rows_mlm_mask_device over the segment plane and the two offset planes, on one stream.  Returns
    (ids, seg, pos, row_first_seq, seq_row, seq_col, nrows, starts, ends, labels[, pred_cells, pred_labels, pred_count]): the masked input ids
    in place of the rows, the packed call's outputs, the offset planes (-1 in cells without a token) and `labels` (ignore_label where nothing
    is predicted); the last three with max_predictions = P > 0 (rows_mlm_mask_device).  The remaining keywords are encode_mlm_batch_device's.
    whole_word=False masks token by token (the planes are returned all the same).  With whole_word=True a row needs cls_id or sep_id: the
    special between two sequences is what keeps a unit from joining the last token of one sequence to the first token of the next when their
    byte offsets happen to be adjacent; without either, ValueError."""
    if whole_word and _special(cls_id) < 0 and _special(sep_id) < 0:
        raise ValueError("encode_packed_mlm_batch_device: whole-word masking over packed rows needs cls_id or sep_id (units could join across sequences)")
    if special_ids is None:
        special_ids = [i for i in (_special(cls_id), _special(sep_id), _special(pad_id)) if i >= 0]
    out = encode_packed_batch_device(h, d_text, d_doc_off, L, cls_id, sep_id, pad_id, unk, rows_cap, return_offsets=True)
    ids, *tail = rows_mlm_mask_device(h, out[0], seg=out[1], starts=out[7] if whole_word else None, ends=out[8] if whole_word else None, nrows=out[6],
                                      special_ids=special_ids, select_prob=select_prob, mask_prob=mask_prob, random_prob=random_prob, mask_id=mask_id,
                                      rand_range=rand_range, ignore_label=ignore_label, seed=seed, epoch=epoch, inplace=True, max_predictions=max_predictions)
    return (ids, *out[1:], *tail)


def denoise_start_prob(noise_density, len_lo=1, len_hi=5):
    """The start_prob of rows_denoise_device for which an interior cell (one with at least len_hi - 1 eligible cells in front of it) is noise
    with probability noise_density.  A cell is noise unless none of the len_hi cells at distance k = 0 .. len_hi - 1 in front of it starts a span
    longer than k:  1 - prod_k (1 - p * P(len > k)) = noise_density,  P(len > k) = 1 for k < len_lo and (len_hi - k) / (len_hi - len_lo + 1) above
    that (lengths are uniform on [len_lo, len_hi]).  The left side rises with p; solved by bisection in double."""
    d, lo, hi = float(noise_density), int(len_lo), int(len_hi)
    if not (0.0 <= d <= 1.0) or not (1 <= lo <= hi):
        raise ValueError("denoise_start_prob: noise_density in [0, 1] and 1 <= len_lo <= len_hi")
    tail = [1.0 if k < lo else (hi - k) / float(hi - lo + 1) for k in range(hi)]

    def density(p):
        clean = 1.0
        for t in tail:
            clean *= 1.0 - p * t
        return 1.0 - clean
    a, b = 0.0, 1.0
    if d <= 0.0:
        return 0.0
    if density(1.0) <= d:
        return 1.0
    for _ in range(200):
        m = 0.5 * (a + b)
        if m == a or m == b:
            break
        if density(m) < d:
            a = m
        else:
            b = m
    return a if abs(density(a) - d) <= abs(density(b) - d) else b


def rows_denoise_device(h, rows, *, mask=None, seg=None, nrows=None, special_ids=(), start_prob, len_lo=1, len_hi=5, sentinel_first, sentinel_step=-1,
                        max_sentinels=100, eos_id=None, pad_id=0, ignore_label=-100, seed, epoch=0, enc_len=None, dec_len=None, return_cells=False, stream=None):
    """Span corruption of rows that are on the device (RowsDenoiseBatchDevice): the encoder inputs and the decoder targets of the T5 / mT5 / UL2
    denoising objective.  -> a dict of int32 tensors: input_ids [R, enc_len] (noise runs collapsed to their sentinels, pad_id behind the row),
    labels [R, dec_len] (every run's sentinel and ids, then eos_id if given, ignore_label behind them), enc_count, dec_count [R] (the
    untruncated lengths) and span_count [R]; with return_cells also enc_cells and dec_cells: the cell of `rows` every copied id came from, -1
    at sentinels, the eos and the padding -- other_plane.gather(1, cells.clamp(min=0).long()) carries any plane of the input into the new layout.
    rows: int32[R, L] from any of the row calls; mask: uint8[R, L] or None; seg: int32[R, L] (the packed or the stream call's segment plane) or
    None: a cell outside the mask or in segment 0 is dropped; a cell holding one of special_ids (at most 8) is copied and ends every span in front
    of it.  An eligible cell starts a span with start_prob (denoise_start_prob gives it for a noise density), of a length uniform on
    [len_lo, len_hi]; run k of a row gets the id sentinel_first + k * sentinel_step, runs past max_sentinels are copied.  nrows: an int64 tensor
    of one element on the device that bounds the rows, or None.  enc_len None = L (always enough), dec_len None = L + 2 (always enough); a row
    longer than a smaller value is cut there and sets BfLastStatus bit 0.  Rows at or past nrows hold pad_id / ignore_label / -1 and counts of 0.
    The result is a function of (seed, epoch, row) and the row alone.  Like every batch call it clears the handle's status word first."""
    import torch
    dev = rows.device
    _dev_i32(rows, dev, "rows_denoise_device: rows")
    _dev_i32(seg, dev, "rows_denoise_device: seg")
    if rows.dim() != 2 or any(t is not None and t.shape != rows.shape for t in (mask, seg)):
        raise ValueError("rows_denoise_device: rows is an [R, L] plane; mask and seg have its shape")
    if mask is not None and (not isinstance(mask, torch.Tensor) or mask.dtype != torch.uint8 or not mask.is_contiguous() or mask.device != dev):
        raise ValueError("rows_denoise_device: mask must be a contiguous torch.uint8 tensor on %s" % dev)
    if nrows is not None and (not isinstance(nrows, torch.Tensor) or nrows.dtype != torch.int64 or nrows.numel() != 1 or nrows.device != dev):
        raise ValueError("rows_denoise_device: nrows must be a torch.int64 tensor of one element on %s" % dev)
    special_ids = [int(x) for x in special_ids]
    if len(special_ids) > 8:
        raise ValueError("rows_denoise_device: at most 8 special ids")
    R, L = rows.shape
    enc_len = L if enc_len is None else int(enc_len)
    dec_len = L + 2 if dec_len is None else int(dec_len)
    if enc_len < 1 or dec_len < 1:
        raise ValueError("rows_denoise_device: enc_len and dec_len are at least 1")
    enc = torch.full((R, enc_len), int(pad_id), dtype=torch.int32, device=dev)
    dec = torch.full((R, dec_len), int(ignore_label), dtype=torch.int32, device=dev)
    counts = [torch.zeros((R,), dtype=torch.int32, device=dev) for _ in range(3)]
    cells = [torch.full((R, n), -1, dtype=torch.int32, device=dev) for n in (enc_len, dec_len)] if return_cells else [None, None]
    s = stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream
    c_special = (c_int32 * max(len(special_ids), 1))(*special_ids)

    def addr(t):
        return None if t is None else t.data_ptr()
    r = lib().RowsDenoiseBatchDevice(c_void_p(h), rows.data_ptr(), L, R, addr(nrows), addr(mask), addr(seg), len(special_ids), c_special, float(start_prob), int(len_lo),
                                     int(len_hi), int(sentinel_first), int(sentinel_step), int(max_sentinels), _special(eos_id), int(pad_id), int(ignore_label),
                                     int(seed) & 0xFFFFFFFFFFFFFFFF, int(epoch) & 0xFFFFFFFF, enc_len, enc.data_ptr(), addr(cells[0]), counts[0].data_ptr(), dec_len,
                                     dec.data_ptr(), addr(cells[1]), counts[1].data_ptr(), counts[2].data_ptr(), c_void_p(s))
    if r != 0:
        raise RuntimeError("RowsDenoiseBatchDevice failed (%d): %s" % (r, lib().BfLastError().decode("utf-8", "replace")))
    out = dict(input_ids=enc, labels=dec, enc_count=counts[0], dec_count=counts[1], span_count=counts[2])
    if return_cells:
        out.update(enc_cells=cells[0], dec_cells=cells[1])
    return out


def encode_denoise_batch_device(h, d_text, d_doc_off, L, eos_id, pad_id, sentinel_first, seed, epoch=0, source="stream", unk=0, start_prob=None, noise_density=0.15,
                                len_lo=1, len_hi=5, sentinel_step=-1, max_sentinels=100, special_ids=None, ignore_label=-100, enc_len=None, dec_len=None,
                                return_cells=False, rows_cap=None, max_ids_per_doc=0x7fffffff):
    """Text in HBM -> the tensors of a span-corruption step, nothing on the host and nothing read back: the tokenizer, a row call and
    rows_denoise_device on one stream.  source="stream": ids_to_stream_rows_batch_device (no bos, eos_id behind every document, the documents laid
    end to end and cut into rows of L cells; its segment plane keeps the padding out and its row count bounds the rows).  source="rows":
    ids_to_rows_batch_device (one row per document, truncated, no cls, eos_id as the closing special; its mask keeps the padding out).
    eos_id and pad_id are the special_ids unless the caller gives others: no span crosses the eos between two documents.  start_prob None:
    denoise_start_prob(noise_density, len_lo, len_hi).  Returns rows_denoise_device's dict with `rows` (the uncorrupted rows), `nrows` (int64, one
    element: the rows that count) and `seg` or `mask` added."""
    if source not in ("stream", "rows"):
        raise ValueError("encode_denoise_batch_device: source is \"stream\" or \"rows\"")
    if _special(eos_id) < 0:
        raise ValueError("encode_denoise_batch_device: eos_id closes every document and is required")
    if special_ids is None:
        special_ids = sorted({int(eos_id), int(pad_id)})
    if start_prob is None:
        start_prob = denoise_start_prob(noise_density, len_lo, len_hi)
    kw = dict(special_ids=special_ids, start_prob=start_prob, len_lo=len_lo, len_hi=len_hi, sentinel_first=sentinel_first, sentinel_step=sentinel_step,
              max_sentinels=max_sentinels, eos_id=eos_id, pad_id=pad_id, ignore_label=ignore_label, seed=seed, epoch=epoch, enc_len=enc_len, dec_len=dec_len,
              return_cells=return_cells)
    if source == "stream":
        d_ids, d_id_off = text_to_ids_batch_device(h, d_text, d_doc_off, int(max_ids_per_doc), unk)
        got = ids_to_stream_rows_batch_device(h, d_ids, d_id_off, L, None, eos_id, pad_id, ignore_label, rows_cap=rows_cap)
        out = rows_denoise_device(h, got[0], seg=got[1], nrows=got[8][:1], **kw)
        out.update(rows=got[0], seg=got[1], nrows=got[8][:1])
        return out
    rows, mask, _, r_off = encode_batch_device(h, d_text, d_doc_off, L, None, eos_id, pad_id, unk)
    out = rows_denoise_device(h, rows, mask=mask, nrows=r_off[-1:], **kw)
    out.update(rows=rows, mask=mask, nrows=r_off[-1:])
    return out


def dict_get_info_batch(h, keys):
    """additive: the reference's FADictInterpreter_t<int>::GetInfo over the model's [pos-dict] for many keys at once (DictGetInfoBatch).
    keys: list of str (code points) or of int sequences, or an (int32 array, int64 offsets) pair.
    Returns (ret int32[nkeys] = value count or -1, info_ids int32[nkeys], values int32[total], value_offsets int64[nkeys+1])."""
    if isinstance(keys, tuple):
        flat, off = keys
    else:
        seqs = [[ord(c) for c in k] if isinstance(k, str) else list(k) for k in keys]
        off = np.zeros(len(seqs) + 1, dtype=np.int64)
        if seqs:
            np.cumsum([len(q) for q in seqs], out=off[1:])
        flat = np.array([c for q in seqs for c in q], dtype=np.int32)
    flat = np.ascontiguousarray(flat, dtype=np.int32)
    off = np.ascontiguousarray(off, dtype=np.int64)
    nk = len(off) - 1
    ret = np.zeros(nk, dtype=np.int32)
    ids = np.zeros(nk, dtype=np.int32)
    v_off = np.zeros(nk + 1, dtype=np.int64)
    L = lib()
    n = L.DictGetInfoBatch(c_void_p(h), flat.ctypes.data, off.ctypes.data, nk, ret.ctypes.data, ids.ctypes.data, None, 0, v_off.ctypes.data)
    vals = np.empty(0, dtype=np.int32)
    if n == -3:                                           # BF_E_CAPACITY: the offsets tell the size
        vals = np.empty(int(v_off[-1]), dtype=np.int32)
        n = L.DictGetInfoBatch(c_void_p(h), flat.ctypes.data, off.ctypes.data, nk, ret.ctypes.data, ids.ctypes.data, vals.ctypes.data, len(vals), v_off.ctypes.data)
    if n < 0:
        raise RuntimeError("DictGetInfoBatch failed: %d (%s)" % (n, L.BfLastError().decode("utf-8", "replace")))
    return ret, ids, vals, v_off


def reserve(h, max_docs, max_bytes, want_offsets=False):
    """additive: size the handle's workspaces once (BfReserve) so that later device-resident batches of that size allocate nothing."""
    r = lib().BfReserve(c_void_p(h), int(max_docs), int(max_bytes), int(bool(want_offsets)))
    if r != 0:
        raise RuntimeError("BfReserve failed (%d): %s" % (r, lib().BfLastError().decode("utf-8", "replace")))


def workspace_grows():
    """diagnostic (BfWorkspaceGrows): (device allocations the library's workspaces and tables have made in this process, those of them for the
    long-document workspace of the words modes, which reserve() leaves out).  A device-resident call on a reserved handle moves neither,
    or only the second."""
    out = (ctypes.c_longlong * 2)()
    r = lib().BfWorkspaceGrows(out)
    if r != 0:
        raise RuntimeError("BfWorkspaceGrows failed (%d)" % r)
    return int(out[0]), int(out[1])


def last_kernel_ms(h):
    """[prep, tokenise, scan, compact, total, dominant kernel] GPU milliseconds of the last batch call (HIP events on its stream)."""
    buf = (c_float * 6)()
    n = lib().BfLastKernelMs(c_void_p(h), buf, 6)
    return [buf[i] for i in range(max(n, 0))]
