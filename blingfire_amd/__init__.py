"""blingfire_amd -- the Python face of the MI355X-native ``libblingfiretokdll.so`` built in-tree by ``blingfire_amd/build.py``.

Three layers, top to bottom of the file:

* the bindings: ``_SIGNATURES``, one ``(restype, argtypes)`` entry per symbol of ``include/blingfiretokdll_amd.h`` (and the three diagnostic
  names of ``csrc/bf_internal.h`` the tests use), applied by ``_bind``; ``tests/test_wrapper_calls.py`` checks the table against the headers;
* the mirror of the reference wrapper ``dist-pypi/blingfire/__init__.py``: same function names, argument meaning and return conventions
  (load_model :229-234, free_model :237-240, text_to_ids :243-253, change_settings_dummy_prefix :287-288, text_to_words :85-102,
  text_to_words_with_model :105-122, the sentence, offsets, hashes, hyphenation and ids_to_text calls);
* what this project adds: the batch forms over host buffers (``*_batch``) and over torch tensors already resident in HBM (``*_batch_device``)
  of the tokenizer and of the secondary calls, the row stage that turns ragged ids into model inputs (rows, pair rows, packed rows, stream
  rows, each with companion planes), the per-row objectives (MLM masking, span corruption), the ``encode_*`` chains that run text to model
  inputs on one stream, and the handle controls (devices, reserve, diagnostics).  The private helpers in front of them hold what these
  share: status checks, input staging, the capacity retry and the count-then-fill drivers of the host and of the Device forms.

There is no CPU fallback: if the shared library is missing or no HIP device is visible the calls
raise / return the reference's error value, loudly.  ``torch`` is imported only inside the functions that need it.
"""
import ctypes
import os
from ctypes import POINTER, byref, c_bool, c_char_p, c_double, c_float, c_int, c_int32, c_int64, c_longlong, c_uint32, c_uint64, c_void_p

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libblingfiretokdll.so")

_lib = None

# ---------------------------------------------------------------------------------------------
# the bindings: symbol -> (restype, argtypes), the mirror of include/blingfiretokdll_amd.h
# ---------------------------------------------------------------------------------------------
_P, _I, _L = c_void_p, c_int, c_int64
_TEXT_TO_IDS = (_I, [_P, c_char_p, _I, _P, _I, _I])
_TEXT_TO_IDS_OFFSETS = (_I, [_P, c_char_p, _I, _P, _P, _P, _I, _I])
_STRING = (_I, [c_char_p, _I, _P, _I])                                # text, its length, the output buffer, its size
_STRING_OFFSETS = (_I, [c_char_p, _I, _P, _P, _P, _I])
_TEXT_BATCH = (_L, [_P, _P, _P, _L, _P, _L, _P])                     # handle, text, offsets, ndocs, text out, its capacity, offsets out
_TEXT_BATCH_DEVICE = (_I, [_P, _P, _P, _L, _L, _P, _L, _P, _P])
_CHARPOS = (_I, [_P, _P, _P, _L, _L, _P, _L, _P, _P, _I, _I, _P, _P, _P, _P])

_SIGNATURES = {
    "GetBlingFireTokVersion": (_I, []),
    "LoadModel": (_P, [c_char_p]),
    "SetModel": (_P, [c_char_p, _I]),
    "FreeModel": (_I, [_P]),
    "SetNoDummyPrefix": (_I, [_P, c_bool]),
    "TextToIds": _TEXT_TO_IDS, "TextToIds_wp": _TEXT_TO_IDS, "TextToIds_sp": _TEXT_TO_IDS,
    "TextToIdsWithOffsets": _TEXT_TO_IDS_OFFSETS, "TextToIdsWithOffsets_wp": _TEXT_TO_IDS_OFFSETS, "TextToIdsWithOffsets_sp": _TEXT_TO_IDS_OFFSETS,
    "TextToIdsBatch": (_L, [_P, _P, _P, _L, _P, _L, _P, _I, _I]),
    "TextToIdsBatchDevice": (_I, [_P, _P, _P, _L, _L, _P, _L, _P, _I, _I, _P]),
    "TextToIdsWithOffsetsBatch": (_L, [_P, _P, _P, _L, _P, _P, _P, _L, _P, _I, _I]),
    "TextToIdsWithOffsetsBatchDevice": (_I, [_P, _P, _P, _L, _L, _P, _P, _P, _L, _P, _I, _I, _P]),
    "TextToWords": _STRING, "TextToSentences": _STRING,
    "TextToWordsWithModel": (_I, _STRING[1] + [_P]), "TextToSentencesWithModel": (_I, _STRING[1] + [_P]),
    "TextToWordsWithOffsets": _STRING_OFFSETS, "TextToSentencesWithOffsets": _STRING_OFFSETS,
    "TextToWordsWithOffsetsWithModel": (_I, _STRING_OFFSETS[1] + [_P]), "TextToSentencesWithOffsetsWithModel": (_I, _STRING_OFFSETS[1] + [_P]),
    "TextToWordsBatch": _TEXT_BATCH, "TextToSentencesBatch": _TEXT_BATCH,
    "TextToWordsBatchDevice": _TEXT_BATCH_DEVICE, "TextToSentencesBatchDevice": _TEXT_BATCH_DEVICE,
    "NormalizeSpaces": (_I, _STRING[1] + [_I]),
    "NormalizeSpacesBatch": (_L, [_P, _P, _L, _P, _L, _P, _I]),
    "TextToHashes": (_I, _STRING[1] + [_I, _I]),
    "TextToHashesBatch": (_L, [_P, _P, _L, _P, _L, _P, _I, _I]),
    "WordHyphenationWithModel": (_I, _STRING[1] + [_P, _I]),
    "WordHyphenationBatch": (_L, _TEXT_BATCH[1] + [_I]),
    "WordHyphenationBatchDevice": (_I, _TEXT_BATCH_DEVICE[1][:-1] + [_I, _P]),
    "IdsToText": (_I, [_P, _P, _I, _P, _I, c_bool]),
    "IdsToTextBatch": (_L, _TEXT_BATCH[1] + [_I]),
    "IdsToTextBatchDevice": (_I, _TEXT_BATCH[1] + [_I, _P]),
    "DictGetInfoBatch": (_L, [_P, _P, _P, _L, _P, _P, _P, _L, _P]),
    "DictGetInfoBatchDevice": (_I, [_P, _P, _P, _L, _P, _P, _P, _L, _P, _P]),
    # the row stage: ragged ids (the Device forms also take their length), the row parameters, the outputs, their capacity, the size answers
    "IdsToRowsBatch": (_L, [_P, _P, _P, _L] + [_I] * 7 + [_P] * 4 + [_L, _P]),
    "IdsToRowsBatchDevice": (_I, [_P, _P, _L, _P, _L] + [_I] * 7 + [_P] * 4 + [_L, _P, _P]),
    "IdsToPairRowsBatch": (_L, [_P, _P, _P, _P, _P, _L] + [_I] * 9 + [_P] * 5 + [_L, _P]),
    "IdsToPairRowsBatchDevice": (_I, [_P, _P, _L, _P, _P, _L, _P, _L] + [_I] * 9 + [_P] * 5 + [_L, _P, _P]),
    "IdsToPackedRowsBatch": (_L, [_P, _P, _P, _L] + [_I] * 5 + [_P] * 4 + [_L, _P, _P]),
    "IdsToPackedRowsBatchDevice": (_I, [_P, _P, _L, _P, _L] + [_I] * 5 + [_P] * 4 + [_L] + [_P] * 4),
    "IdsToStreamRowsBatch": (_L, [_P, _P, _P, _L] + [_I] * 6 + [_P] * 6 + [_L, _P, _P]),
    "IdsToStreamRowsBatchDevice": (_I, [_P, _P, _L, _P, _L] + [_I] * 6 + [_P] * 6 + [_L] + [_P] * 4),
    "RowsSpanCellsBatchDevice": (_I, [_P, _P, _P, _I, _L, _P, _P, _L, _P, _P, _I, _P, _P, _P]),
    "RowsMlmMaskBatchDevice": (_I, [_P, _P, _I, _L] + [_P] * 5 + [_I, _P] + [c_double] * 3 + [_I] * 4 + [c_uint64, c_uint32, _P, _P, _P]),
    "RowsDenoiseBatchDevice": (_I, [_P, _P, _I, _L] + [_P] * 3 + [_I, _P, c_double] + [_I] * 8 + [c_uint64, c_uint32] + [_I, _P, _P, _P] * 2 + [_P, _P]),
    # offsets in characters: handle, text, doc offsets, ndocs, total bytes, item offsets, items cap, starts, ends, unit, flags, the three outputs, stream
    "ByteToCharOffsetsBatchDevice": _CHARPOS, "CharToByteOffsetsBatchDevice": _CHARPOS,
    "BfLastKernelMs": (_I, [_P, POINTER(c_float), _I]),
    "BfLastStatus": (_I, [_P]),
    "BfLastError": (c_char_p, []),
    "BfBpeFallbackDocs": (c_longlong, [_P]),
    "BfModelKind": (_I, [_P]),
    "BfReserve": (_I, [_P, _L, _L, _I]),
    "BfSetBpePoolBytes": (_L, [_P, _L]),
    "BfSetDevices": (_I, [_P, _P, _I]),
    "BfShardHandle": (_P, [_P, _I]),
    "BfShardRanges": (_I, [_P, _L, _I, _P]),
    # declared in csrc/bf_internal.h: diagnostics the tests and tools drive
    "BfSetVariant": (_I, [_P, _I]),
    "BfSetLexStats": (_I, [_P, _I]),
    "BfWorkspaceGrows": (_I, [_P]),
}
# a ...Planes... call is its base call plus (nplanes, one source array per side, fill, planes out), in front of the stream of a Device form
for _base in ("IdsToRowsBatch", "IdsToPairRowsBatch", "IdsToPackedRowsBatch"):
    _tail = [_I] + [_P] * (4 if "Pair" in _base else 3)
    for _dev in ("", "Device"):
        _res, _args = _SIGNATURES[_base + _dev]
        _SIGNATURES[_base.replace("RowsBatch", "RowsPlanesBatch") + _dev] = (_res, _args[:-1] + _tail + _args[-1:] if _dev else _args + _tail)
_SIGNATURES["RowsMlmPredictionsBatchDevice"] = (_I, _SIGNATURES["RowsMlmMaskBatchDevice"][1][:-1] + [_I, _P, _P, _P, _P])


def _bind(L):
    """applies _SIGNATURES to a loaded library (or to what stands in for one in a test) and returns it"""
    for name, (restype, argtypes) in _SIGNATURES.items():
        f = getattr(L, name)
        f.restype, f.argtypes = restype, argtypes
    return L


def lib():
    """The loaded C-ABI library (built by blingfire_amd/build.py)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("%s is missing: run `python -m blingfire_amd.build` (hipcc, gfx950) first; "
                               "there is no CPU fallback" % LIB_PATH)
        _lib = _bind(ctypes.CDLL(LIB_PATH))
    return _lib


# ---------------------------------------------------------------------------------------------
# shared helpers
# ---------------------------------------------------------------------------------------------
_COUNT = "%s failed: %d (%s)"                   # the message of the host calls that answer a count; the Device and control calls use _check's default


def _last_error():
    return lib().BfLastError().decode("utf-8", "replace")


def _check(name, r, ok, layout="%s failed (%d): %s"):
    if not ok:
        raise RuntimeError(layout % (name, r, _last_error()))


def _special(i):
    return -1 if i is None else int(i)


def _nspecial(*ids):
    """how many of the special ids there are (None or negative = none)"""
    return sum(1 for i in ids if _special(i) >= 0)


def _default_special_ids(*ids):
    return [i for i in map(_special, ids) if i >= 0]


def _seed_args(seed, epoch):
    return int(seed) & 0xFFFFFFFFFFFFFFFF, int(epoch) & 0xFFFFFFFF


def _ids_cap(total, ndocs, max_len):
    """the ids `ndocs` documents of `total` bytes can give: every id covers >= 1 element of <= 2*(n+1) per document"""
    return min(2 * (total + ndocs), ndocs * max(max_len, 0))


def pack_docs(docs):
    """list of str/bytes -> (uint8 array, int64 offsets[ndocs+1])"""
    bs = [d.encode("utf-8") if isinstance(d, str) else bytes(d) for d in docs]
    off = np.zeros(len(bs) + 1, dtype=np.int64)
    if bs:
        np.cumsum([len(b) for b in bs], out=off[1:])
    text = np.frombuffer(b"".join(bs), dtype=np.uint8) if bs else np.zeros(0, dtype=np.uint8)
    return text, off


def _host_ragged(items, off, dtype=np.int32):
    """-> (items, offsets, n): contiguous arrays of `dtype` and int64, and the number of ranges"""
    off = np.ascontiguousarray(off, dtype=np.int64)
    return np.ascontiguousarray(items, dtype=dtype), off, len(off) - 1


def _host_docs(docs):
    """list of str / bytes, or a (uint8 array, int64 offsets) pair -> _host_ragged of the text"""
    return _host_ragged(*(docs if isinstance(docs, tuple) else pack_docs(docs)), dtype=np.uint8)


def _upload_docs(docs):
    """_host_docs, uploaded with torch to the current device -> (text, offsets) tensors"""
    import torch
    text, off, _ = _host_docs(docs)
    return torch.from_numpy(text.copy()).cuda(), torch.from_numpy(off.copy()).cuda()


def _stream_arg(stream, dev):
    """the caller's raw stream handle, or torch's current stream on `dev`"""
    import torch
    return c_void_p(stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream)


def _dev_addr(t):
    return None if t is None else t.data_ptr()


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


def _string_call(name, s, mul, add, *post):
    """the reference's single-string calls: `s` into a buffer of mul * bytes + add -> the string the library wrote, '' on error or if it does not fit"""
    s_bytes = s.encode("utf-8")
    o = ctypes.create_string_buffer(len(s_bytes) * mul + add)
    n = getattr(lib(), name)(s_bytes, len(s_bytes), o, len(o), *post)
    return "" if n == -1 or n > len(o) else o.value.decode("utf-8")


def _spans_call(name, s, h, mul, count):
    """the reference's ...WithOffsets calls: (string, [(begin, end) per unit]) with the library's byte offsets (end inclusive) turned into character
    offsets into `s` (end exclusive); count(string) = the units there are"""
    s_bytes = s.encode("utf-8")
    cap = len(s_bytes) * mul
    o = ctypes.create_string_buffer(max(cap, 1))
    st = (c_int32 * max(cap, 1))()
    en = (c_int32 * max(cap, 1))()
    n = getattr(lib(), name)(s_bytes, len(s_bytes), o, byref(st), byref(en), cap, c_void_p(h) if h else None)
    if n == -1 or n > cap:
        return "", []
    text = o.value.decode("utf-8")
    lead = np.frombuffer(s_bytes, dtype=np.uint8) & 0xC0 != 0x80
    char_at = np.concatenate([[0], np.cumsum(lead)])          # byte offset -> number of characters that start before it
    return text, [(int(char_at[st[i]]), int(char_at[en[i] + 1])) for i in range(count(text) if text else 0)]


def _capacity_retry(name, pre, post, dtype, n):
    """the host calls that size their own output: fn(*pre, out, capacity, offsets, *post) with no output first; on BF_E_CAPACITY (-3) the offsets
    tell the size and the call is made again.  -> (out, offsets int64[n + 1])"""
    fn = getattr(lib(), name)
    out, off = np.empty(0, dtype=dtype), np.zeros(n + 1, dtype=np.int64)
    r = fn(*pre, None, 0, off.ctypes.data, *post)
    if r == -3:
        out = np.empty(int(off[-1]), dtype=dtype)
        r = fn(*pre, out.ctypes.data, len(out), off.ctypes.data, *post)
    _check(name, r, r >= 0, _COUNT)
    return out, off


# The outputs a row call has in front of its capacity: (dtype, an [R, L] plane or an [R] vector, entries beyond R).
_PLANE, _MASK, _VEC = ("int32", True, 0), ("uint8", True, 0), ("int32", False, 0)
_ROWS_OUTS = (_PLANE, _MASK, _VEC, _VEC)                              # rows, mask, row item, row first id
_PAIR_OUTS = (_PLANE, _MASK, _MASK, _VEC, _VEC)                       # rows, mask, type, row pair, row first B id
_PACKED_OUTS = (_PLANE,) * 3 + (("int32", False, 1),)                 # rows, seg, pos, row_first_seq[R + 1]
_STREAM_OUTS = (_PLANE,) * 4 + (_VEC,) * 2                            # rows, seg, pos, labels, row first seq, row first pos


def _outs(spec, n, L, dev=None):
    """the outputs of `spec` for n rows: numpy arrays, or torch tensors on `dev`"""
    shapes = [((n + more, L) if plane else (n + more,), t) for t, plane, more in spec]
    if dev is None:
        return [np.empty(shape, dtype=t) for shape, t in shapes]
    import torch
    return [torch.empty(shape, dtype=getattr(torch, t), device=dev) for shape, t in shapes]


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


def _planes_host(sides, fill):
    return _plane_tail([[_np_i32(x) for x in side] for side in sides], fill, lambda a: a.ctypes.data)


def _planes_device(sides, fill, dev, what):
    """what: one "function: argument[%d]" per side, for the message that refuses a source"""
    return _plane_tail([[_dev_i32(t, dev, w % k) for k, t in enumerate(side)] for w, side in zip(what, sides)], fill, lambda t: t.data_ptr())


def _pair_sides(src_a, src_b, n):
    return [list(src_a) if src_a is not None else [None] * n, list(src_b) if src_b is not None else [None] * n]


def _planes_name(name, extra):
    return name.replace("RowsBatch", "RowsPlanesBatch") if extra else name


def _count_fill_host(name, pre, spec, L, answers, fill_empty, extra=None):
    """the host forms of the row stage (count_fill_host of bf_capi.cpp, seen from outside): fn(*pre, outputs of `spec`, capacity, *answers[, planes])
    with every output NULL at capacity 0 answers the row count R -- `answers` (sized by the items, not by the rows) are filled by that call already
    -- then the outputs are allocated and the call is made again; with R = 0 only if `fill_empty`.  extra = (nplanes, tail) of _plane_tail: the
    ...Planes symbol, whose int32 [R, L] planes are appended to the result as a list.  -> (*outputs, *answers[, planes])"""
    name = _planes_name(name, extra)
    fn = getattr(lib(), name)
    nextra, tail = extra if extra else (0, lambda outs: ())
    after = [a.ctypes.data for a in answers]
    n = fn(*pre, *[None] * len(spec), 0, *after, *tail(None))
    _check(name, n, n >= 0, _COUNT)
    outs = _outs(spec, n, L)
    more = _outs((_PLANE,) * nextra, n, L)
    if n > 0 or fill_empty:
        r = fn(*pre, *[o.ctypes.data for o in outs], n, *after, *tail(more))
        _check(name, r, r == n, _COUNT)
    return (*outs, *answers, more) if extra else (*outs, *answers)


def _count_fill_device(name, pre, spec, L, seq, total, rows_cap, dev, stream, extra=None):
    """the Device forms of the row stage that may have to ask for their size: fn(*pre, outputs of `spec`, capacity, *seq, total[, planes], stream);
    `seq` = the outputs sized by the items, `total` = the int64 tensor whose last element is the row count.  rows_cap None: a size query (every
    output NULL at capacity 0) whose total is read back.  extra: as in _count_fill_host.  -> (outputs, planes)"""
    import torch
    name = _planes_name(name, extra)
    fn = getattr(lib(), name)
    nextra, tail = extra if extra else (0, lambda outs: ())
    s = _stream_arg(stream, dev)

    def call(outs, cap, seq_outs, more=None):
        r = fn(*pre, *outs, cap, *seq_outs, total.data_ptr(), *tail(more), s)
        _check(name, r, r == 0)
    if rows_cap is None:
        call([None] * len(spec), 0, [None] * len(seq))
        if stream is not None:
            torch.cuda.synchronize(dev)                   # (a raw stream handle: nothing finer to wait on)
        rows_cap = int(total[-1].item())
    outs = _outs(spec, rows_cap, L, dev)
    more = _outs((_PLANE,) * nextra, rows_cap, L, dev)
    call([o.data_ptr() for o in outs], rows_cap, [t.data_ptr() for t in seq], more)
    return outs, more


def _head(h, nseq, *ragged):
    """the leading arguments of a call over ragged ids: the handle, (ids, offsets) of every side -- numpy arrays, or torch tensors for the Device
    forms, which also take the length of the ids -- and the number of sequences"""
    args = [c_void_p(h)]
    for ids, off in ragged:
        args += [ids.ctypes.data, off.ctypes.data] if isinstance(ids, np.ndarray) else [ids.data_ptr(), ids.numel(), off.data_ptr()]
    return (*args, nseq)


def _rows_args(L, cls_id, sep_id, pad_id, stride, max_rows_per_seq, pad_left):
    return (int(L), _special(cls_id), _special(sep_id), int(pad_id), int(stride), int(max_rows_per_seq), int(bool(pad_left)))


def _pair_args(L, cls_id, sep_id, pad_id, mode, max_a, stride, max_rows_per_pair, pad_left, double_sep):
    return (int(L), _special(cls_id), _special(sep_id), int(pad_id), int(mode), int(max_a), int(stride), int(max_rows_per_pair),
            (1 if pad_left else 0) | (2 if double_sep else 0))


def _packed_args(L, cls_id, sep_id, pad_id):
    return (int(L), _special(cls_id), _special(sep_id), int(pad_id), 0)


def _stream_args(L, bos_id, eos_id, pad_id, ignore_label, drop_last, pos_from_row, labels_within_doc):
    return (int(L), _special(bos_id), _special(eos_id), int(pad_id), int(ignore_label),
            (1 if drop_last else 0) | (2 if pos_from_row else 0) | (4 if labels_within_doc else 0))


# ---------------------------------------------------------------------------------------------
# the mirror of the reference wrapper
# ---------------------------------------------------------------------------------------------

def get_blingfiretok_version():
    return lib().GetBlingFireTokVersion()


def load_model(file_name):
    """reference __init__.py:229-234; raises instead of returning a NULL handle."""
    h = lib().LoadModel(file_name.encode("utf-8"))
    if not h:
        raise RuntimeError("LoadModel(%r) failed: %s" % (file_name, _last_error()))
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
    return _string_call("NormalizeSpaces", s, 2, 4, uSpace)


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
    return _string_call("WordHyphenationWithModel", s, 4, 1, c_void_p(h) if h else None, uHy)


def word_hyphenation_batch(h, words, uHy=0x2D):
    """additive: word_hyphenation_with_model over many words (str or bytes) in one call -> list of str; '' where the single call fails."""
    text, off, nw = _host_ragged(*pack_docs(words), dtype=np.uint8)
    out, t_off = _capacity_retry("WordHyphenationBatch", (c_void_p(h), text.ctypes.data, off.ctypes.data, nw), (uHy,), np.uint8, nw)
    raw = out.tobytes()
    return [raw[t_off[i]:t_off[i + 1]].decode("utf-8") for i in range(nw)]


def text_to_words(s):
    """reference __init__.py:85-102: space-joined words by the built-in wbd.bin; '' on error."""
    return _string_call("TextToWords", s, 3, 0)


def text_to_words_with_model(h, s):
    """reference __init__.py:105-122"""
    return _string_call("TextToWordsWithModel", s, 3, 0, c_void_p(h))


def text_to_words_with_offsets(s, h=None):
    """reference __init__.py:161-223: (string, [(begin, end) per word]) as character offsets into `s`, end exclusive."""
    return _spans_call("TextToWordsWithOffsetsWithModel", s, h, 3, lambda words: len(words.split(" ")))


def text_to_sentences(s):
    """reference __init__.py:45-62: one sentence per line by the built-in sbd.bin; '' on error."""
    return _string_call("TextToSentences", s, 2, 0)


def text_to_sentences_with_model(h, s):
    """reference __init__.py:65-82"""
    return _string_call("TextToSentencesWithModel", s, 2, 0, c_void_p(h))


def text_to_sentences_and_offsets(s, h=None):
    """reference __init__.py:225-226: (string, [(begin, end) per sentence]) as character offsets into `s`, end exclusive."""
    return _spans_call("TextToSentencesWithOffsetsWithModel", s, h, 2, lambda sents: sents.count("\n") + 1)


def text_to_sentences_batch(docs, h=None):
    """additive: TextToSentences over many documents; h None = the built-in sbd.bin.  Same conventions as text_to_words_batch."""
    return text_to_words_batch(docs, h, _fn="TextToSentencesBatch")


def text_to_words_batch(docs, h=None, _fn="TextToWordsBatch"):
    """additive: TextToWords over many documents (list of bytes, or a (text uint8, offsets int64) pair) -> (text uint8, offsets int64[ndocs+1]);
    h None = the built-in wbd.bin."""
    text, off, nd = _host_docs(docs)
    return _capacity_retry(_fn, (c_void_p(h) if h else None, text.ctypes.data, off.ctypes.data, nd), (), np.uint8, nd)


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
    ids, id_off, nseq = _host_ragged(ids, id_off)
    return _capacity_retry("IdsToTextBatch", (c_void_p(h), ids.ctypes.data, id_off.ctypes.data, nseq), (int(bool(skip_special_tokens)),), np.uint8, nseq)


def change_settings_dummy_prefix(h, add_prefix):
    lib().SetNoDummyPrefix(c_void_p(h), bool(not add_prefix))


# ---------------------------------------------------------------------------------------------
# additive batch API
# ---------------------------------------------------------------------------------------------

def set_devices(h, device_ids):
    """Range-shards the host-buffer batch calls of h over the listed devices of this node (BfSetDevices: tables replicated, contiguous
    byte-balanced document ranges, one host thread per device, no collective).  A device may be listed more than once."""
    arr = (c_int * len(device_ids))(*[int(d) for d in device_ids])
    r = lib().BfSetDevices(c_void_p(h), arr, len(device_ids))
    _check("BfSetDevices", r, r == 0)


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
    text, off, ndocs = _host_docs(docs)
    cap = _ids_cap(int(off[-1] - off[0]) if ndocs > 0 else 0, ndocs, max_len) + 1
    ids = np.empty(cap, dtype=np.int32)
    id_off = np.zeros(ndocs + 1, dtype=np.int64)
    r = lib().TextToIdsBatch(c_void_p(h), text.ctypes.data, off.ctypes.data, ndocs, ids.ctypes.data, cap, id_off.ctypes.data,
                             max_len, unk)
    _check("TextToIdsBatch", r, r >= 0)
    return ids[:r], id_off


def text_to_ids_with_offsets_batch(h, docs, max_len, unk=0):
    """Batch form of TextToIdsWithOffsets: (ids, starts, ends, id_offsets); starts/ends are byte offsets inside each document."""
    text, off, ndocs = _host_docs(docs)
    cap = _ids_cap(int(off[-1] - off[0]) if ndocs > 0 else 0, ndocs, max_len) + 1
    ids, starts, ends = (np.empty(cap, dtype=np.int32) for _ in range(3))
    id_off = np.zeros(ndocs + 1, dtype=np.int64)
    r = lib().TextToIdsWithOffsetsBatch(c_void_p(h), text.ctypes.data, off.ctypes.data, ndocs, ids.ctypes.data, starts.ctypes.data,
                                        ends.ctypes.data, cap, id_off.ctypes.data, max_len, unk)
    _check("TextToIdsWithOffsetsBatch", r, r >= 0)
    return ids[:r], starts[:r], ends[:r], id_off


def text_to_ids_batch_device(h, d_text, d_doc_off, max_len, unk=0, out_ids=None, out_off=None, stream=None):
    """Device-resident batch: torch uint8 text tensor + int64 offsets tensor (both on the model's GPU).

    Enqueues on torch's current stream (or `stream`) and returns (ids int32[cap], id_offsets int64[ndocs+1]) tensors
    without synchronising; the valid id count is id_offsets[-1].
    """
    import torch
    ndocs = d_doc_off.numel() - 1
    total = d_text.numel()
    if out_ids is None:
        out_ids = torch.empty(max(1, _ids_cap(total, ndocs, max_len)), dtype=torch.int32, device=d_text.device)
    if out_off is None:
        out_off = torch.empty(ndocs + 1, dtype=torch.int64, device=d_text.device)
    r = lib().TextToIdsBatchDevice(c_void_p(h), d_text.data_ptr(), d_doc_off.data_ptr(), ndocs, total, out_ids.data_ptr(),
                                   out_ids.numel(), out_off.data_ptr(), max_len, unk, _stream_arg(stream, d_text.device))
    _check("TextToIdsBatchDevice", r, r == 0)
    return out_ids, out_off


def text_to_ids_with_offsets_batch_device(h, d_text, d_doc_off, max_len, unk=0, stream=None):
    """Device-resident text_to_ids_with_offsets_batch, the mirror of text_to_ids_batch_device: (ids int32[cap], starts int32[cap],
    ends int32[cap], id_offsets int64[ndocs+1]) tensors, enqueued without synchronising; starts / ends are byte offsets inside each
    document (the end inclusive), the valid count is id_offsets[-1]."""
    import torch
    ndocs = d_doc_off.numel() - 1
    total = d_text.numel()
    cap = max(1, _ids_cap(total, ndocs, max_len))
    ids, starts, ends = (torch.empty(cap, dtype=torch.int32, device=d_text.device) for _ in range(3))
    out_off = torch.empty(ndocs + 1, dtype=torch.int64, device=d_text.device)
    r = lib().TextToIdsWithOffsetsBatchDevice(c_void_p(h), d_text.data_ptr(), d_doc_off.data_ptr(), ndocs, total, ids.data_ptr(), starts.data_ptr(),
                                              ends.data_ptr(), cap, out_off.data_ptr(), max_len, unk, _stream_arg(stream, d_text.device))
    _check("TextToIdsWithOffsetsBatchDevice", r, r == 0)
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
    r = lib().IdsToTextBatchDevice(c_void_p(h), d_ids.data_ptr(), d_id_off.data_ptr(), nseq, out_text.data_ptr(), out_text.numel(),
                                   out_off.data_ptr(), int(bool(skip_special_tokens)), _stream_arg(stream, d_ids.device))
    _check("IdsToTextBatchDevice", r, r == 0)
    return out_text, out_off


def _rows_host(name, pre, nseq, L, spec, planes):
    """the host forms of rows and pair rows; planes = None (the base symbol) or (sources per side, fill)"""
    r_off = np.zeros(nseq + 1, dtype=np.int64)
    return _count_fill_host(name, pre, spec, L, [r_off], False, planes and _planes_host(*planes))


def _rows_device(name, pre, nseq, L, spec, one_row, rows_cap, dev, stream, planes, what=()):
    """the Device forms of rows and pair rows.  rows_cap None: nseq rows where one row per item is certain (`one_row`), else a size query whose
    total is read back.  planes, what: as in _rows_host and _planes_device"""
    import torch
    extra = planes and _planes_device(*planes, dev, what)
    r_off = torch.empty(nseq + 1, dtype=torch.int64, device=dev)
    if rows_cap is None and one_row:
        rows_cap = nseq
    outs, more = _count_fill_device(name, pre, spec, L, [], r_off, rows_cap, dev, stream, extra)
    return (*outs, r_off, more) if extra else (*outs, r_off)


def _ids_to_rows(h, ids, id_off, L, args, planes=None):
    ids, id_off, nseq = _host_ragged(ids, id_off)
    return _rows_host("IdsToRowsBatch", _head(h, nseq, (ids, id_off)) + args, nseq, L, _ROWS_OUTS, planes)


def _ids_to_rows_device(h, d_ids, d_id_off, L, args, one_row, rows_cap, stream, planes=None):
    nseq = d_id_off.numel() - 1
    return _rows_device("IdsToRowsBatchDevice", _head(h, nseq, (d_ids, d_id_off)) + args, nseq, L, _ROWS_OUTS, one_row, rows_cap, d_ids.device, stream,
                              planes, ["ids_to_rows_planes_batch_device: src[%d]"])


def ids_to_rows_batch(h, ids, id_off, L, cls_id=None, sep_id=None, pad_id=0, stride=0, max_rows_per_seq=1, pad_left=False):
    """additive: ragged ids (int32 array + int64 offsets[nseq+1]) -> fixed-shape model inputs (IdsToRowsBatch).  A sequence longer than
    the row is cut into windows that share `stride` ids (max_rows_per_seq: 1 = truncate, 0 = every window); cls_id / sep_id None = no
    such special.  Returns (rows int32[R, L], mask uint8[R, L], row_seq int32[R], row_first int32[R], row_offsets int64[nseq+1]):
    the rows of sequence q are [row_offsets[q], row_offsets[q+1]), row_first is the index within its sequence of a row's first id."""
    return _ids_to_rows(h, ids, id_off, L, _rows_args(L, cls_id, sep_id, pad_id, stride, max_rows_per_seq, pad_left))


def ids_to_rows_batch_device(h, d_ids, d_id_off, L, cls_id=None, sep_id=None, pad_id=0, stride=0, max_rows_per_seq=1, pad_left=False,
                             rows_cap=None, stream=None):
    """Device-resident ids_to_rows_batch: torch int32 ids + int64 offsets on one GPU (text_to_ids_batch_device's results as they are) ->
    the same five results as tensors on that device, enqueued on torch's current stream (or `stream`).  rows_cap None: nseq rows when
    max_rows_per_seq is 1 (nothing is read back); otherwise a size query whose total is read back (one synchronisation).  With a
    rows_cap of the caller's the tensors have rows_cap rows, row_offsets[-1] of them valid; rows beyond it are dropped (BfLastStatus bit 0)."""
    return _ids_to_rows_device(h, d_ids, d_id_off, L, _rows_args(L, cls_id, sep_id, pad_id, stride, max_rows_per_seq, pad_left), max_rows_per_seq == 1,
                               rows_cap, stream)


def ids_to_rows_planes_batch(h, ids, id_off, L, cls_id=None, sep_id=None, pad_id=0, stride=0, max_rows_per_seq=1, pad_left=False, src=(), fill=()):
    """ids_to_rows_batch with companion planes (IdsToRowsPlanesBatch): src = up to 4 int32 arrays parallel to ids (token offsets, labels, ...),
    fill = one int per array.  Returns ids_to_rows_batch's five results and the list of planes, int32[R, L] each: a cell that holds an id holds
    that id's element of the array, every other cell the array's fill."""
    return _ids_to_rows(h, ids, id_off, L, _rows_args(L, cls_id, sep_id, pad_id, stride, max_rows_per_seq, pad_left), ([src], fill))


def ids_to_rows_planes_batch_device(h, d_ids, d_id_off, L, cls_id=None, sep_id=None, pad_id=0, stride=0, max_rows_per_seq=1, pad_left=False,
                                    rows_cap=None, stream=None, src=(), fill=()):
    """Device-resident ids_to_rows_planes_batch: src = int32 tensors on the device of d_ids, parallel to it (the starts / ends of
    text_to_ids_with_offsets_batch_device as they are).  Returns ids_to_rows_batch_device's five results and the list of plane tensors."""
    return _ids_to_rows_device(h, d_ids, d_id_off, L, _rows_args(L, cls_id, sep_id, pad_id, stride, max_rows_per_seq, pad_left), max_rows_per_seq == 1,
                               rows_cap, stream, ([src], fill))


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
    r = lib().RowsSpanCellsBatchDevice(c_void_p(h), starts.data_ptr(), ends.data_ptr(), L, R,
                                       None if row_offsets is None else row_offsets.data_ptr() + 8 * nseq, _dev_addr(row_seq),
                                       nseq, span_first.data_ptr(), span_last.data_ptr(), int(none_cell), out[0].data_ptr(), out[1].data_ptr(), _stream_arg(stream, dev))
    _check("RowsSpanCellsBatchDevice", r, r == 0)
    return out[0], out[1]


_OFFSET_UNITS = {"char": 0, "utf16": 1}


def _charpos_device(name, h, d_text, d_doc_off, starts, ends, item_off, unit, ends_in_exclusive, ends_out_exclusive, items_cap, stream, return_doc_units, in_place):
    """the two offset conversions: one argument list, one result layout"""
    import torch
    if unit not in _OFFSET_UNITS:
        raise ValueError("%s: unit is 'char' (code points) or 'utf16' (UTF-16 code units), not %r" % (name, unit))
    dev = d_text.device
    ndocs = d_doc_off.numel() - 1
    what = name + ": %s"
    starts, ends = _dev_i32(starts, dev, what % "starts"), _dev_i32(ends, dev, what % "ends")
    if item_off is not None and (item_off.dtype != torch.int64 or not item_off.is_contiguous() or item_off.device != dev or item_off.numel() != ndocs + 1):
        raise ValueError("%s: item_off must be a contiguous torch.int64 tensor of ndocs + 1 entries on %s" % (name, dev))
    if starts is not None and ends is not None and starts.numel() != ends.numel():
        raise ValueError("%s: starts and ends name different numbers of items" % name)
    given = starts if starts is not None else ends
    if items_cap is None:
        items_cap = 0 if given is None else given.numel()
    elif given is not None and items_cap > given.numel():
        raise ValueError("%s: items_cap is beyond the arrays" % name)
    outs = [None if t is None else t if in_place else torch.empty_like(t) for t in (starts, ends)]
    units = torch.empty(ndocs, dtype=torch.int32, device=dev) if return_doc_units else None
    fn = "ByteToCharOffsetsBatchDevice" if name.startswith("byte") else "CharToByteOffsetsBatchDevice"
    r = getattr(lib(), fn)(c_void_p(h), d_text.data_ptr(), d_doc_off.data_ptr(), ndocs, d_text.numel(), _dev_addr(item_off), int(items_cap), _dev_addr(starts), _dev_addr(ends),
                           _OFFSET_UNITS[unit], (1 if ends_in_exclusive else 0) | (2 if ends_out_exclusive else 0), _dev_addr(outs[0]), _dev_addr(outs[1]), _dev_addr(units),
                           _stream_arg(stream, dev))
    _check(fn, r, r == 0)
    return (*outs, units) if return_doc_units else tuple(outs)


def byte_to_char_offsets_device(h, d_text, d_doc_off, starts=None, ends=None, item_off=None, unit="char", ends_in_exclusive=False, ends_out_exclusive=False, items_cap=None,
                                stream=None, return_doc_units=False, in_place=False):
    """Byte offsets inside documents that are in HBM -> offsets in code points (unit "char": what a Python str indexes by) or in UTF-16 code units
    ("utf16": C#, JS), on the device (ByteToCharOffsetsBatchDevice).  starts / ends: int32 tensors of one entry per item, either may be None;
    item_off: the int64[ndocs+1] offsets that say which document an item belongs to (text_to_ids_with_offsets_batch_device's id offsets as they
    are; the items at or past its last entry are left alone), or None: item d belongs to document d.  Ends are inclusive on both sides unless
    ends_in_exclusive / ends_out_exclusive say otherwise.  A negative entry (a dummy prefix, a plane's fill) gives -1; a position beyond its document
    gives -1 and BfLastStatus bit 3.  Returns (starts, ends) -- None where none was given; new tensors, or the inputs with in_place -- and with
    return_doc_units also doc_units int32[ndocs], every document's length in the unit.  Enqueued on torch's current stream (or `stream`); nothing
    is read back.  Any loaded handle serves; the model is not consulted."""
    return _charpos_device("byte_to_char_offsets_device", h, d_text, d_doc_off, starts, ends, item_off, unit, ends_in_exclusive, ends_out_exclusive, items_cap, stream,
                           return_doc_units, in_place)


def char_to_byte_offsets_device(h, d_text, d_doc_off, starts=None, ends=None, item_off=None, unit="char", ends_in_exclusive=False, ends_out_exclusive=False, items_cap=None,
                                stream=None, return_doc_units=False, in_place=False):
    """The inverse of byte_to_char_offsets_device (CharToByteOffsetsBatchDevice): offsets in code points or UTF-16 code units -> byte offsets, the
    first byte of the character that holds the unit (an index on a low surrogate gives its character's first byte); an exclusive end one past
    the document's last unit gives the document's length.  Same arguments and results; doc_units is again the length in the unit."""
    return _charpos_device("char_to_byte_offsets_device", h, d_text, d_doc_off, starts, ends, item_off, unit, ends_in_exclusive, ends_out_exclusive, items_cap, stream,
                           return_doc_units, in_place)


def _offset_keywords(fn_name, offset_unit, offset_end, return_offsets=True):
    """checks the offset_unit / offset_end keywords of an encode_* call -> True when the offsets are to be converted"""
    if offset_unit not in ("byte", "char", "utf16") or offset_end not in ("inclusive", "exclusive"):
        raise ValueError("%s: offset_unit is 'byte', 'char' or 'utf16' and offset_end 'inclusive' or 'exclusive'" % fn_name)
    if offset_unit == "byte":
        if offset_end != "inclusive":
            raise ValueError("%s: offset_end='exclusive' needs offset_unit 'char' or 'utf16' (byte offsets stay as the tokenizer gives them)" % fn_name)
        return False
    if not return_offsets:
        raise ValueError("%s: offset_unit=%r without return_offsets" % (fn_name, offset_unit))
    return True


def _ragged_offsets_in_units(h, d_text, d_doc_off, d_st, d_en, d_id_off, offset_unit, offset_end):
    """the tokenizer's ragged starts / ends, converted where they lie: once per token, before the planes are gathered from them"""
    byte_to_char_offsets_device(h, d_text, d_doc_off, d_st, d_en, d_id_off, unit=offset_unit, ends_out_exclusive=offset_end == "exclusive", in_place=True)


def encode_batch_device(h, d_text, d_doc_off, L, cls_id, sep_id, pad_id, unk=0, stride=0, max_rows_per_doc=1, pad_left=False, return_offsets=False,
                        offset_unit="byte", offset_end="inclusive"):
    """Text in HBM -> tensors a model takes, nothing on the host: text_to_ids_batch_device and ids_to_rows_batch_device on one stream.
    Every document is tokenised up to the ids its rows can hold (all of them when max_rows_per_doc is 0).
    Returns (rows int32[R, L], mask uint8[R, L], row_doc int32[R], row_offsets int64[ndocs+1]); with return_offsets also
    (starts int32[R, L], ends int32[R, L]): every token's first and last byte in its document, -1 in cells without a token.
    offset_unit "char" / "utf16": the planes count code points / UTF-16 code units instead of bytes (byte_to_char_offsets_device on the ragged
    offsets, between the tokenizer call and the planes call; the default "byte" is today's call sequence unchanged); offset_end "exclusive": the
    ends are one past the token's last unit, so that text[s:e] is the token.  "exclusive" needs offset_unit "char" or "utf16": with "byte" it is
    refused (ValueError) -- byte offsets stay exactly as the tokenizer gives them -- and so is a unit other than "byte" without return_offsets.
    BfLastStatus afterwards is that of the last call on the handle, the planes call, as before; the conversion's own word (it has nothing to report
    on the tokenizer's offsets) is cleared by it."""
    body = int(L) - _nspecial(cls_id, sep_id)
    step = body - int(stride)
    if body < 1 or stride < 0 or step < 1 or max_rows_per_doc < 0:
        raise ValueError("encode_batch_device: L leaves no room for ids, or stride / max_rows_per_doc are out of range")
    convert = _offset_keywords("encode_batch_device", offset_unit, offset_end, return_offsets)
    max_len = min(body + (max_rows_per_doc - 1) * step, 2 ** 31 - 1) if max_rows_per_doc > 0 else 2 ** 31 - 1
    if return_offsets:
        d_ids, d_st, d_en, d_id_off = text_to_ids_with_offsets_batch_device(h, d_text, d_doc_off, max_len, unk)
        if convert:
            _ragged_offsets_in_units(h, d_text, d_doc_off, d_st, d_en, d_id_off, offset_unit, offset_end)
        rows, mask, seq, _, r_off, (st, en) = ids_to_rows_planes_batch_device(h, d_ids, d_id_off, L, cls_id, sep_id, pad_id, stride, max_rows_per_doc, pad_left,
                                                                               src=[d_st, d_en], fill=[-1, -1])
        return rows, mask, seq, r_off, st, en
    d_ids, d_id_off = text_to_ids_batch_device(h, d_text, d_doc_off, max_len, unk)
    rows, mask, seq, _, r_off = ids_to_rows_batch_device(h, d_ids, d_id_off, L, cls_id, sep_id, pad_id, stride, max_rows_per_doc, pad_left)
    return rows, mask, seq, r_off


def encode_batch(h, docs, L, cls_id, sep_id, pad_id, unk=0, stride=0, max_rows_per_doc=1, pad_left=False):
    """encode_batch_device for a list of str / bytes (or a (uint8 array, int64 offsets) pair): packed, uploaded with torch to the current
    device, encoded there."""
    return encode_batch_device(h, *_upload_docs(docs), L, cls_id, sep_id, pad_id, unk, stride, max_rows_per_doc, pad_left)


def _ids_to_pair_rows(fn_name, h, ids_a, off_a, ids_b, off_b, L, args, planes=None):
    ids_a, off_a, nseq = _host_ragged(ids_a, off_a)
    ids_b, off_b, nseq_b = _host_ragged(ids_b, off_b)
    if nseq_b != nseq:
        raise ValueError("%s: off_a and off_b name different numbers of sequences" % fn_name)
    return _rows_host("IdsToPairRowsBatch", _head(h, nseq, (ids_a, off_a), (ids_b, off_b)) + args, nseq, L, _PAIR_OUTS, planes)


def _ids_to_pair_rows_device(fn_name, h, d_ids_a, d_off_a, d_ids_b, d_off_b, L, args, one_row, rows_cap, stream, planes=None):
    nseq = d_off_a.numel() - 1
    if d_off_b.numel() != nseq + 1:
        raise ValueError("%s: d_off_a and d_off_b name different numbers of sequences" % fn_name)
    return _rows_device("IdsToPairRowsBatchDevice", _head(h, nseq, (d_ids_a, d_off_a), (d_ids_b, d_off_b)) + args, nseq, L, _PAIR_OUTS, one_row, rows_cap,
                              d_ids_a.device, stream, planes, [fn_name + ": src_a[%d]", fn_name + ": src_b[%d]"])


def ids_to_pair_rows_batch(h, ids_a, off_a, ids_b, off_b, L, cls_id=None, sep_id=None, pad_id=0, mode=1, max_a=0, stride=0, max_rows_per_pair=1,
                           pad_left=False, double_sep=False):
    """additive: pairs of ragged ids (two int32 arrays + two int64 offsets[nseq+1]) -> [cls] A [sep] B [sep] rows with type ids
    (IdsToPairRowsBatch).  mode 1: one row per pair, ids dropped from the end of the longer side until both fit (max_a, stride and
    max_rows_per_pair stay at their defaults).  mode 0: the first max_a ids of A in every row, B cut into windows that share `stride` ids
    (max_rows_per_pair: 1 = truncate B, 0 = every window).  double_sep: two separators between A and B.  Returns (rows int32[R, L],
    mask uint8[R, L], type uint8[R, L], row_pair int32[R], row_first_b int32[R], row_offsets int64[nseq+1]): the rows of pair q are
    [row_offsets[q], row_offsets[q+1]), row_first_b is the index within B of a row's first B id."""
    return _ids_to_pair_rows("ids_to_pair_rows_batch", h, ids_a, off_a, ids_b, off_b, L,
                             _pair_args(L, cls_id, sep_id, pad_id, mode, max_a, stride, max_rows_per_pair, pad_left, double_sep))


def ids_to_pair_rows_batch_device(h, d_ids_a, d_off_a, d_ids_b, d_off_b, L, cls_id=None, sep_id=None, pad_id=0, mode=1, max_a=0, stride=0,
                                  max_rows_per_pair=1, pad_left=False, double_sep=False, rows_cap=None, stream=None):
    """Device-resident ids_to_pair_rows_batch: torch int32 ids + int64 offsets of both sides on one GPU (the results of two
    text_to_ids_batch_device calls as they are; the same tensor may serve both sides) -> the same six results as tensors on that device,
    enqueued on torch's current stream (or `stream`).  rows_cap None: nseq rows when one row per pair is certain (mode 1, or
    max_rows_per_pair 1: nothing is read back); otherwise a size query whose total is read back (one synchronisation).  With a rows_cap of
    the caller's the tensors have rows_cap rows, row_offsets[-1] of them valid; rows beyond it are dropped (BfLastStatus bit 0)."""
    return _ids_to_pair_rows_device("ids_to_pair_rows_batch_device", h, d_ids_a, d_off_a, d_ids_b, d_off_b, L,
                                    _pair_args(L, cls_id, sep_id, pad_id, mode, max_a, stride, max_rows_per_pair, pad_left, double_sep),
                                    mode == 1 or max_rows_per_pair == 1, rows_cap, stream)


def ids_to_pair_rows_planes_batch(h, ids_a, off_a, ids_b, off_b, L, cls_id=None, sep_id=None, pad_id=0, mode=1, max_a=0, stride=0, max_rows_per_pair=1,
                                  pad_left=False, double_sep=False, src_a=None, src_b=None, fill=()):
    """ids_to_pair_rows_batch with companion planes (IdsToPairRowsPlanesBatch): src_a / src_b = lists of int32 arrays parallel to ids_a / ids_b,
    one entry per fill value; a list that is None, or an entry that is, leaves that side's cells at the fill.  Returns ids_to_pair_rows_batch's
    six results and the list of planes, int32[R, L] each."""
    return _ids_to_pair_rows("ids_to_pair_rows_planes_batch", h, ids_a, off_a, ids_b, off_b, L,
                             _pair_args(L, cls_id, sep_id, pad_id, mode, max_a, stride, max_rows_per_pair, pad_left, double_sep),
                             (_pair_sides(src_a, src_b, len(fill)), fill))


def ids_to_pair_rows_planes_batch_device(h, d_ids_a, d_off_a, d_ids_b, d_off_b, L, cls_id=None, sep_id=None, pad_id=0, mode=1, max_a=0, stride=0,
                                         max_rows_per_pair=1, pad_left=False, double_sep=False, rows_cap=None, stream=None, src_a=None, src_b=None, fill=()):
    """Device-resident ids_to_pair_rows_planes_batch: src_a / src_b = lists of int32 tensors parallel to d_ids_a / d_ids_b (None entries and
    None lists allowed).  Returns ids_to_pair_rows_batch_device's six results and the list of plane tensors."""
    return _ids_to_pair_rows_device("ids_to_pair_rows_planes_batch_device", h, d_ids_a, d_off_a, d_ids_b, d_off_b, L,
                                    _pair_args(L, cls_id, sep_id, pad_id, mode, max_a, stride, max_rows_per_pair, pad_left, double_sep),
                                    mode == 1 or max_rows_per_pair == 1, rows_cap, stream, (_pair_sides(src_a, src_b, len(fill)), fill))


def encode_pairs_batch_device(h, d_text_a, d_off_a, d_text_b, d_off_b, L, cls_id, sep_id, pad_id, unk=0, mode=1, max_a=0, stride=0, max_rows_per_pair=1,
                              pad_left=False, double_sep=False, return_offsets=False, offsets_a=False, offset_unit="byte", offset_end="inclusive"):
    """Two texts in HBM -> the tensors a pair model takes, nothing on the host: two text_to_ids_batch_device calls and
    ids_to_pair_rows_batch_device on one stream.  Each side is tokenised up to the ids its rows can hold: T = L - specials for both in mode 1
    (cutting both to T first does not change what longest-first keeps); in mode 0 max_a for A and T + (max_rows_per_pair - 1) * (T - stride)
    for B (all of B when max_rows_per_pair is 0).
    Returns (rows int32[R, L], mask uint8[R, L], type uint8[R, L], row_pair int32[R], row_first_b int32[R], row_offsets int64[npairs+1]); with
    return_offsets also (starts int32[R, L], ends int32[R, L]): first and last byte of every token of B in its text (with offsets_a, of A in
    its own text too), -1 in every other cell.  offset_unit / offset_end: as in encode_batch_device, every side against its own text
    (offset_end="exclusive" with offset_unit="byte" is refused there and here)."""
    nsep = 0 if _special(sep_id) < 0 else 3 if double_sep else 2
    T = int(L) - _nspecial(cls_id) - nsep
    if T < 1 or mode not in (0, 1) or (mode == 0 and not (0 <= max_a <= T - 1 and 0 <= stride < T - max_a and max_rows_per_pair >= 0)):
        raise ValueError("encode_pairs_batch_device: L leaves no room for ids, or mode / max_a / stride / max_rows_per_pair are out of range")
    convert = _offset_keywords("encode_pairs_batch_device", offset_unit, offset_end, return_offsets)
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
            if convert:
                _ragged_offsets_in_units(h, d_text_a, d_off_a, d_st_a, d_en_a, d_idoff_a, offset_unit, offset_end)
        else:
            d_ids_a, d_idoff_a = text_to_ids_batch_device(h, d_text_a, d_off_a, len_a, unk)
        d_ids_b, d_st_b, d_en_b, d_idoff_b = text_to_ids_with_offsets_batch_device(h, d_text_b, d_off_b, len_b, unk)
        if convert:
            _ragged_offsets_in_units(h, d_text_b, d_off_b, d_st_b, d_en_b, d_idoff_b, offset_unit, offset_end)
        *base, (st, en) = ids_to_pair_rows_planes_batch_device(h, d_ids_a, d_idoff_a, d_ids_b, d_idoff_b, L, cls_id, sep_id, pad_id, mode, max_a, stride,
                                                              max_rows_per_pair, pad_left, double_sep, src_a=src_a, src_b=[d_st_b, d_en_b], fill=[-1, -1])
        return (*base, st, en)
    d_ids_a, d_idoff_a = text_to_ids_batch_device(h, d_text_a, d_off_a, len_a, unk)
    d_ids_b, d_idoff_b = text_to_ids_batch_device(h, d_text_b, d_off_b, len_b, unk)
    return ids_to_pair_rows_batch_device(h, d_ids_a, d_idoff_a, d_ids_b, d_idoff_b, L, cls_id, sep_id, pad_id, mode, max_a, stride, max_rows_per_pair,
                                         pad_left, double_sep)


def encode_qa_batch_device(h, d_text_q, d_off_q, d_text_c, d_off_c, L, cls_id, sep_id, pad_id, max_q, stride, unk=0, double_sep=False, d_ans_first=None,
                           d_ans_last=None, offset_unit="byte", offset_end="inclusive", answer_unit="byte"):
    """Questions and contexts in HBM -> extractive-QA inputs, one stream end to end: [cls] question [sep] context window [sep] rows (mode 0,
    the first max_q question ids in every row, every window of the context, `stride` ids shared by neighbours) with the context's byte
    offsets as planes.  Returns (rows, mask, type, row_pair, row_first_b, row_offsets, starts, ends) -- starts / ends int32[R, L]: first and
    last byte of every context token in its context, -1 elsewhere -- and, with d_ans_first / d_ans_last (int32[npairs]: first and last byte,
    inclusive, of each answer in its context; negative = none), also (start_cell, end_cell) int32[R]: the token cells of the answer in every
    row, the [cls] cell (0) in both where the answer is not inside the row's window.  The only read-back is the size query of
    ids_to_pair_rows_batch_device.  BfLastStatus afterwards is that of the LAST call on the handle alone, as always: with answers that is the span
    call, which cleared what the tokenizer and row calls reported (ids or rows dropped, bad ranges); a caller who needs those runs
    encode_pairs_batch_device(..., return_offsets=True) and rows_span_cells_device itself and reads the status between them.
    answer_unit "char" / "utf16": the answers are the first and the last character (code point / UTF-16 code unit), inclusive, of each answer in
    its context -- a SQuAD answer_start as it stands; they go through char_to_byte_offsets_device (one item per context) in front of the span
    call, which compares them with byte planes.  offset_unit / offset_end: the planes returned count characters, as in encode_batch_device;
    with answers they are converted behind the span call (the cells of a context's rows as its items), without answers on the ragged offsets.
    With answers AND offset_unit "char" / "utf16" the last call on the handle is that conversion of the planes: BfLastStatus afterwards is its own
    word, and what the span call reported (bit 3) is cleared like everything before it.  offset_end="exclusive" needs offset_unit "char" or
    "utf16": with "byte" it is refused (ValueError), byte offsets stay as the tokenizer gives them."""
    convert = _offset_keywords("encode_qa_batch_device", offset_unit, offset_end)
    if answer_unit not in ("byte", "char", "utf16"):
        raise ValueError("encode_qa_batch_device: answer_unit is 'byte', 'char' or 'utf16'")
    if d_ans_first is None or d_ans_last is None:
        return encode_pairs_batch_device(h, d_text_q, d_off_q, d_text_c, d_off_c, L, cls_id, sep_id, pad_id, unk, 0, max_q, stride, 0, False, double_sep,
                                         return_offsets=True, offset_unit=offset_unit, offset_end=offset_end)
    out = encode_pairs_batch_device(h, d_text_q, d_off_q, d_text_c, d_off_c, L, cls_id, sep_id, pad_id, unk, 0, max_q, stride, 0, False, double_sep,
                                    return_offsets=True)
    if answer_unit != "byte":
        import torch
        first, last = (t.to(device=d_text_c.device, dtype=torch.int32).contiguous() for t in (d_ans_first, d_ans_last))
        d_ans_first, d_ans_last = char_to_byte_offsets_device(h, d_text_c, d_off_c, first, last, unit=answer_unit)
    cells = rows_span_cells_device(h, out[6], out[7], out[3], out[5], d_ans_first, d_ans_last, 0)
    if convert:
        byte_to_char_offsets_device(h, d_text_c, d_off_c, out[6].view(-1), out[7].view(-1), out[5] * int(L), unit=offset_unit,
                                    ends_out_exclusive=offset_end == "exclusive", in_place=True)
    return (*out, *cells)


def encode_pairs_batch(h, docs_a, docs_b, L, cls_id, sep_id, pad_id, unk=0, mode=1, max_a=0, stride=0, max_rows_per_pair=1, pad_left=False, double_sep=False):
    """encode_pairs_batch_device for two lists of str / bytes (or two (uint8 array, int64 offsets) pairs): packed, uploaded with torch to the
    current device, encoded there."""
    return encode_pairs_batch_device(h, *_upload_docs(docs_a), *_upload_docs(docs_b), L, cls_id, sep_id, pad_id, unk, mode, max_a, stride, max_rows_per_pair,
                                     pad_left, double_sep)


def _ids_to_packed_rows(h, ids, id_off, L, cls_id, sep_id, pad_id, planes=None):
    """the host forms of the packed call; unlike _rows_host the second call is made for R = 0 too: row_first_seq has R + 1 entries"""
    ids, id_off, nseq = _host_ragged(ids, id_off)
    seq = [np.empty(nseq, dtype=np.int32) for _ in range(2)]
    return _count_fill_host("IdsToPackedRowsBatch", _head(h, nseq, (ids, id_off)) + _packed_args(L, cls_id, sep_id, pad_id), _PACKED_OUTS, L, seq, True,
                            planes and _planes_host(*planes))


def ids_to_packed_rows_batch(h, ids, id_off, L, cls_id=None, sep_id=None, pad_id=0):
    """additive: ragged ids (int32 array + int64 offsets[nseq+1]) -> PACKED model inputs (IdsToPackedRowsBatch): several sequences share a
    row, filled greedily and in order; a sequence longer than a row is truncated, none is split.  cls_id / sep_id None = no such special.
    Returns (rows int32[R, L], seg int32[R, L], pos int32[R, L], row_first_seq int32[R + 1], seq_row int32[nseq], seq_col int32[nseq]):
    seg numbers the sequences of a row from 1 (0 = padding), pos restarts at every sequence, row r holds the sequences
    [row_first_seq[r], row_first_seq[r + 1]), and sequence q begins at cell seq_col[q] of row seq_row[q]."""
    return _ids_to_packed_rows(h, ids, id_off, L, cls_id, sep_id, pad_id)


def ids_to_packed_rows_planes_batch(h, ids, id_off, L, cls_id=None, sep_id=None, pad_id=0, src=(), fill=()):
    """ids_to_packed_rows_batch with companion planes (IdsToPackedRowsPlanesBatch): src = up to 4 int32 arrays parallel to ids (token offsets,
    labels, ...), fill = one int per array.  Returns ids_to_packed_rows_batch's six results and the list of planes, int32[R, L] each: a cell
    that holds an id holds that id's element of the array, every other cell (cls_id, sep_id, padding) the array's fill."""
    return _ids_to_packed_rows(h, ids, id_off, L, cls_id, sep_id, pad_id, ([src], fill))


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
    extra = None if planes is None else _planes_device([planes], () if fill is None else fill, dev, ["ids_to_packed_rows_batch_device: planes[%d]"])
    nrows = torch.empty(1, dtype=torch.int64, device=dev)
    seq = [torch.empty(nseq, dtype=torch.int32, device=dev) for _ in range(2)]
    outs, more = _count_fill_device("IdsToPackedRowsBatchDevice", _head(h, nseq, (d_ids, d_id_off)) + _packed_args(L, cls_id, sep_id, pad_id), _PACKED_OUTS, L, seq,
                                    nrows, rows_cap, dev, stream, extra)
    return (*outs, *seq, nrows, *more)


def encode_packed_batch_device(h, d_text, d_doc_off, L, cls_id, sep_id, pad_id, unk=0, rows_cap=None, return_offsets=False, offset_unit="byte",
                               offset_end="inclusive"):
    """Text in HBM -> packed tensors a model takes, nothing on the host: text_to_ids_batch_device (every document tokenised up to the ids
    a row can hold) and ids_to_packed_rows_batch_device on one stream.  Returns what ids_to_packed_rows_batch_device returns; with a
    rows_cap of the caller's nothing is read back.  With return_offsets also (starts int32[R, L], ends int32[R, L]) behind nrows: every
    token's first and last byte in its document, -1 in cells without a token.  offset_unit / offset_end: as in encode_batch_device
    (offset_end="exclusive" with offset_unit="byte" is refused there and here)."""
    body = int(L) - _nspecial(cls_id, sep_id)
    if body < 1:
        raise ValueError("encode_packed_batch_device: L leaves no room for ids")
    convert = _offset_keywords("encode_packed_batch_device", offset_unit, offset_end, return_offsets)
    if return_offsets:
        d_ids, d_st, d_en, d_id_off = text_to_ids_with_offsets_batch_device(h, d_text, d_doc_off, body, unk)
        if convert:
            _ragged_offsets_in_units(h, d_text, d_doc_off, d_st, d_en, d_id_off, offset_unit, offset_end)
        return ids_to_packed_rows_batch_device(h, d_ids, d_id_off, L, cls_id, sep_id, pad_id, rows_cap, planes=[d_st, d_en], fill=[-1, -1])
    d_ids, d_id_off = text_to_ids_batch_device(h, d_text, d_doc_off, body, unk)
    return ids_to_packed_rows_batch_device(h, d_ids, d_id_off, L, cls_id, sep_id, pad_id, rows_cap)


def encode_packed_batch(h, docs, L, cls_id, sep_id, pad_id, unk=0, rows_cap=None):
    """encode_packed_batch_device for a list of str / bytes (or a (uint8 array, int64 offsets) pair): packed into one buffer, uploaded with
    torch to the current device, encoded there."""
    return encode_packed_batch_device(h, *_upload_docs(docs), L, cls_id, sep_id, pad_id, unk, rows_cap)


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
    ids, id_off, nseq = _host_ragged(ids, id_off)
    seq = [np.empty(nseq, dtype=np.int32) for _ in range(2)]
    pre = _head(h, nseq, (ids, id_off)) + _stream_args(L, bos_id, eos_id, pad_id, ignore_label, drop_last, pos_from_row, labels_within_doc)
    return _count_fill_host("IdsToStreamRowsBatch", pre, _STREAM_OUTS, L, seq, True)


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
        rows_cap = -(-(d_ids.numel() + _nspecial(bos_id, eos_id) * nseq) // L) if L > 0 else 0
    outs = _outs(_STREAM_OUTS, rows_cap, L, dev)
    seq = [torch.empty(nseq, dtype=torch.int32, device=dev) for _ in range(2)]
    nrows = torch.empty(2, dtype=torch.int64, device=dev)
    pre = _head(h, nseq, (d_ids, d_id_off)) + _stream_args(L, bos_id, eos_id, pad_id, ignore_label, drop_last, pos_from_row, labels_within_doc)
    r = lib().IdsToStreamRowsBatchDevice(*pre, *[t.data_ptr() for t in outs], rows_cap, *[t.data_ptr() for t in seq], nrows.data_ptr(), _stream_arg(stream, dev))
    _check("IdsToStreamRowsBatchDevice", r, r == 0)
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
    return encode_clm_batch_device(h, *_upload_docs(docs), L, bos_id, eos_id, pad_id, unk, ignore_label, drop_last, pos_from_row, labels_within_doc, rows_cap,
                                   max_ids_per_doc)


def _row_inputs(fn_name, rows, mask, seg, nrows, special_ids, **int32_planes):
    """what the per-row objectives check of their inputs: `rows`, `seg` and the further planes int32 on one device, `mask` uint8, all of one [R, L]
    shape, `nrows` one int64 on the device, at most 8 special ids.  -> (device, R, L, the special ids as (count, int32 array))"""
    import torch
    dev = rows.device
    for what, t in (("rows", rows), ("seg", seg), *int32_planes.items()):
        _dev_i32(t, dev, "%s: %s" % (fn_name, what))
    if rows.dim() != 2 or any(t is not None and t.shape != rows.shape for t in (mask, seg, *int32_planes.values())):
        names = ["mask", "seg", *int32_planes]
        raise ValueError("%s: rows is an [R, L] plane; %s and %s have its shape" % (fn_name, ", ".join(names[:-1]), names[-1]))
    if mask is not None and (not isinstance(mask, torch.Tensor) or mask.dtype != torch.uint8 or not mask.is_contiguous() or mask.device != dev):
        raise ValueError("%s: mask must be a contiguous torch.uint8 tensor on %s" % (fn_name, dev))
    if nrows is not None and (not isinstance(nrows, torch.Tensor) or nrows.dtype != torch.int64 or nrows.numel() != 1 or nrows.device != dev):
        raise ValueError("%s: nrows must be a torch.int64 tensor of one element on %s" % (fn_name, dev))
    special_ids = [int(x) for x in special_ids]
    if len(special_ids) > 8:
        raise ValueError("%s: at most 8 special ids" % fn_name)
    return dev, *rows.shape, (len(special_ids), (c_int32 * max(len(special_ids), 1))(*special_ids))


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
    dev, R, L, special = _row_inputs("rows_mlm_mask_device", rows, mask, seg, nrows, special_ids, starts=starts, ends=ends)
    if (starts is None) != (ends is None):
        raise ValueError("rows_mlm_mask_device: starts and ends come together")
    if isinstance(max_predictions, bool) or not isinstance(max_predictions, (int, np.integer)) or max_predictions < 0:
        raise ValueError("rows_mlm_mask_device: max_predictions is an integer >= 0")
    P = int(max_predictions)
    if P > 0 and (L > 4096 or P > 1 << 20):
        raise ValueError("rows_mlm_mask_device: max_predictions needs rows of at most 4096 cells and is at most 1 << 20")
    ids = rows if inplace else rows.clone()
    labels = torch.full((R, L), int(ignore_label), dtype=torch.int32, device=dev)
    s = _stream_arg(stream, dev)
    common = (c_void_p(h), rows.data_ptr(), L, R, _dev_addr(nrows), _dev_addr(mask), _dev_addr(seg), _dev_addr(starts), _dev_addr(ends), *special,
              float(select_prob), float(mask_prob), float(random_prob), int(mask_id), int(rand_range[0]), int(rand_range[1]), int(ignore_label),
              *_seed_args(seed, epoch), ids.data_ptr(), labels.data_ptr())
    if P > 0:
        cells = torch.zeros((R, P), dtype=torch.int32, device=dev)
        plabels = torch.full((R, P), int(ignore_label), dtype=torch.int32, device=dev)
        count = torch.zeros((R,), dtype=torch.int32, device=dev)
        r = lib().RowsMlmPredictionsBatchDevice(*common, P, cells.data_ptr(), plabels.data_ptr(), count.data_ptr(), s)
        _check("RowsMlmPredictionsBatchDevice", r, r == 0)
        return ids, labels, cells, plabels, count
    r = lib().RowsMlmMaskBatchDevice(*common, s)
    _check("RowsMlmMaskBatchDevice", r, r == 0)
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
    three forms (rows_mlm_mask_device).  The offset planes stay in bytes (there is no offset_unit here): the whole-word rule is byte adjacency."""
    if packed and whole_word:
        raise ValueError("encode_mlm_batch_device: packed rows have no offset planes, so no whole-word masking")
    if special_ids is None:
        special_ids = _default_special_ids(cls_id, sep_id, pad_id)
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
    byte offsets happen to be adjacent; without either, ValueError.  The planes stay in bytes (no offset_unit): the whole-word rule is byte adjacency."""
    if whole_word and _nspecial(cls_id, sep_id) == 0:
        raise ValueError("encode_packed_mlm_batch_device: whole-word masking over packed rows needs cls_id or sep_id (units could join across sequences)")
    if special_ids is None:
        special_ids = _default_special_ids(cls_id, sep_id, pad_id)
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
    dev, R, L, special = _row_inputs("rows_denoise_device", rows, mask, seg, nrows, special_ids)
    enc_len = L if enc_len is None else int(enc_len)
    dec_len = L + 2 if dec_len is None else int(dec_len)
    if enc_len < 1 or dec_len < 1:
        raise ValueError("rows_denoise_device: enc_len and dec_len are at least 1")
    enc = torch.full((R, enc_len), int(pad_id), dtype=torch.int32, device=dev)
    dec = torch.full((R, dec_len), int(ignore_label), dtype=torch.int32, device=dev)
    counts = [torch.zeros((R,), dtype=torch.int32, device=dev) for _ in range(3)]
    cells = [torch.full((R, n), -1, dtype=torch.int32, device=dev) for n in (enc_len, dec_len)] if return_cells else [None, None]
    r = lib().RowsDenoiseBatchDevice(c_void_p(h), rows.data_ptr(), L, R, _dev_addr(nrows), _dev_addr(mask), _dev_addr(seg), *special, float(start_prob), int(len_lo),
                                     int(len_hi), int(sentinel_first), int(sentinel_step), int(max_sentinels), _special(eos_id), int(pad_id), int(ignore_label),
                                     *_seed_args(seed, epoch), enc_len, enc.data_ptr(), _dev_addr(cells[0]), counts[0].data_ptr(), dec_len,
                                     dec.data_ptr(), _dev_addr(cells[1]), counts[1].data_ptr(), counts[2].data_ptr(), _stream_arg(stream, dev))
    _check("RowsDenoiseBatchDevice", r, r == 0)
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
    flat, off, nk = _host_ragged(flat, off)
    ret = np.zeros(nk, dtype=np.int32)                    # the two per-key outputs: the size pass fills them already
    ids = np.zeros(nk, dtype=np.int32)
    vals, v_off = _capacity_retry("DictGetInfoBatch", (c_void_p(h), flat.ctypes.data, off.ctypes.data, nk, ret.ctypes.data, ids.ctypes.data), (), np.int32, nk)
    return ret, ids, vals, v_off


def reserve(h, max_docs, max_bytes, want_offsets=False):
    """additive: size the handle's workspaces once (BfReserve) so that later device-resident batches of that size allocate nothing."""
    r = lib().BfReserve(c_void_p(h), int(max_docs), int(max_bytes), int(bool(want_offsets)))
    _check("BfReserve", r, r == 0)


def workspace_grows():
    """diagnostic (BfWorkspaceGrows): (device allocations the library's workspaces and tables have made in this process, those of them for the
    long-document workspace of the words modes, which reserve() leaves out).  A device-resident call on a reserved handle moves neither,
    or only the second."""
    out = (c_longlong * 2)()
    r = lib().BfWorkspaceGrows(out)
    if r != 0:
        raise RuntimeError("BfWorkspaceGrows failed (%d)" % r)
    return int(out[0]), int(out[1])


def last_kernel_ms(h):
    """[prep, tokenise, scan, compact, total, dominant kernel] GPU milliseconds of the last batch call (HIP events on its stream)."""
    buf = (c_float * 6)()
    n = lib().BfLastKernelMs(c_void_p(h), buf, 6)
    return [buf[i] for i in range(max(n, 0))]
