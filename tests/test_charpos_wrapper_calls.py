"""CPU: what the offset-conversion wrappers and the offset_unit / offset_end / answer_unit keywords send to the C library, call by call, against
the recording stand-in of test_wrapper_calls.py (no built library, model or device)."""
import pytest

from test_wrapper_calls import N, P, dev_docs, env, raises, writes_total  # noqa: F401  (env is the fixture)


def names(L):
    return [n for n, _ in L.log]


def test_offset_conversion_calls(env):
    bf, L, torch = env.bf, env.L, env.torch
    d_text, d_off = dev_docs(torch)
    st, en = torch.tensor([0, 1, 0], dtype=torch.int32), torch.tensor([0, 1, 0], dtype=torch.int32)
    ioff = torch.tensor([0, 2, 3], dtype=torch.int64)
    L.script.update(ByteToCharOffsetsBatchDevice=[0, 0, 0, -2], CharToByteOffsetsBatchDevice=[0])
    s, e = bf.byte_to_char_offsets_device(7, d_text, d_off, st, en, ioff)
    assert s is not st and e is not en and s.shape == st.shape and s.dtype == torch.int32
    s, e, u = bf.byte_to_char_offsets_device(7, d_text, d_off, st, None, unit="utf16", ends_out_exclusive=True, return_doc_units=True, in_place=True, stream=9)
    assert s is st and e is None and tuple(u.shape) == (2,) and u.dtype == torch.int32
    (u,) = bf.byte_to_char_offsets_device(7, d_text, d_off, return_doc_units=True, stream=9)[2:]
    raises(RuntimeError, "ByteToCharOffsetsBatchDevice failed (-2): boom", bf.byte_to_char_offsets_device, 7, d_text, d_off, st, en, ioff, stream=9)
    bf.char_to_byte_offsets_device(7, d_text, d_off, st, en, ioff, ends_in_exclusive=True, items_cap=2, stream=9)
    assert L.log == [("ByteToCharOffsetsBatchDevice", (P, P, P, 2, 3, P, 3, P, P, 0, 0, P, P, N, P)),
                     ("ByteToCharOffsetsBatchDevice", (P, P, P, 2, 3, N, 3, P, N, 1, 2, P, N, P, P)),
                     ("ByteToCharOffsetsBatchDevice", (P, P, P, 2, 3, N, 0, N, N, 0, 0, N, N, P, P)),
                     ("ByteToCharOffsetsBatchDevice", (P, P, P, 2, 3, P, 3, P, P, 0, 0, P, P, N, P)), ("BfLastError", ()),
                     ("CharToByteOffsetsBatchDevice", (P, P, P, 2, 3, P, 2, P, P, 0, 1, P, P, N, P))]
    for bad in (dict(unit="byte"), dict(starts=st.long()), dict(item_off=ioff[:2]), dict(item_off=ioff.int()), dict(ends=en[:2]), dict(items_cap=4)):
        kw = dict(dict(starts=st, ends=en, item_off=ioff), **bad)
        with pytest.raises(ValueError):
            bf.byte_to_char_offsets_device(7, d_text, d_off, **kw)


def test_encode_keywords_place_the_conversion_between_the_tokenizer_and_the_planes(env):
    bf, L, torch = env.bf, env.L, env.torch
    d_text, d_off = dev_docs(torch)
    L.script.update(IdsToRowsPlanesBatchDevice=[0, 0], IdsToPackedRowsPlanesBatchDevice=[0], IdsToPairRowsPlanesBatchDevice=[0])
    out = bf.encode_batch_device(7, d_text, d_off, 4, 101, 102, 0, return_offsets=True, offset_unit="char", offset_end="exclusive")
    assert len(out) == 6
    assert names(L) == ["TextToIdsWithOffsetsBatchDevice", "ByteToCharOffsetsBatchDevice", "IdsToRowsPlanesBatchDevice"]
    conv = L.log[1][1]
    assert conv[3:5] == (2, 3) and conv[5] == P and conv[7:11] == (P, P, 0, 2) and conv[13] is N                  # item offsets given; char, exclusive ends out; no doc units
    assert L.raw[1][1][7] == L.raw[1][1][11] and L.raw[1][1][8] == L.raw[1][1][12]                               # in place, on the ragged arrays
    del L.log[:], L.raw[:]
    bf.encode_batch_device(7, d_text, d_off, 4, 101, 102, 0, return_offsets=True)                                 # the default: today's sequence
    assert names(L) == ["TextToIdsWithOffsetsBatchDevice", "IdsToRowsPlanesBatchDevice"]
    del L.log[:], L.raw[:]
    bf.encode_packed_batch_device(7, d_text, d_off, 4, 101, 102, 0, rows_cap=1, return_offsets=True, offset_unit="utf16")
    assert names(L) == ["TextToIdsWithOffsetsBatchDevice", "ByteToCharOffsetsBatchDevice", "IdsToPackedRowsPlanesBatchDevice"] and L.log[1][1][9:11] == (1, 0)
    del L.log[:], L.raw[:]
    bf.encode_pairs_batch_device(7, d_text, d_off, d_text, d_off, 8, 101, 102, 0, return_offsets=True, offsets_a=True, offset_unit="char")
    assert names(L) == ["TextToIdsWithOffsetsBatchDevice", "ByteToCharOffsetsBatchDevice", "TextToIdsWithOffsetsBatchDevice", "ByteToCharOffsetsBatchDevice",
                        "IdsToPairRowsPlanesBatchDevice"]
    for fn, kw in ((bf.encode_batch_device, dict(return_offsets=True, offset_unit="bytes")), (bf.encode_batch_device, dict(return_offsets=True, offset_end="exclusive")),
                   (bf.encode_batch_device, dict(offset_unit="char")), (bf.encode_packed_batch_device, dict(offset_unit="utf16"))):
        with pytest.raises(ValueError):
            fn(7, d_text, d_off, 4, 101, 102, 0, **kw)


def test_qa_answers_in_characters(env):
    bf, L, torch = env.bf, env.L, env.torch
    d_text, d_off = dev_docs(torch)
    q = writes_total(23, 2, 2)
    L.script.update(IdsToPairRowsPlanesBatchDevice=[q, 0, q, 0, q, 0])
    ans = torch.tensor([0, 1], dtype=torch.int64)
    args = (7, d_text, d_off, d_text, d_off, 8, 101, 102, 0, 2, 1)
    chain = ["TextToIdsBatchDevice", "TextToIdsWithOffsetsBatchDevice", "IdsToPairRowsPlanesBatchDevice", "IdsToPairRowsPlanesBatchDevice"]
    out = bf.encode_qa_batch_device(*args, d_ans_first=ans, d_ans_last=ans, answer_unit="char")
    assert len(out) == 10 and names(L) == chain + ["CharToByteOffsetsBatchDevice", "RowsSpanCellsBatchDevice"]
    inv = L.log[4][1]
    assert inv[3:7] == (2, 3, N, 2) and inv[9:11] == (0, 0)                                                       # one item per context, ends inclusive on both sides
    del L.log[:], L.raw[:]
    out = bf.encode_qa_batch_device(*args, d_ans_first=ans, d_ans_last=ans, answer_unit="utf16", offset_unit="char", offset_end="exclusive")
    assert names(L) == chain + ["CharToByteOffsetsBatchDevice", "RowsSpanCellsBatchDevice", "ByteToCharOffsetsBatchDevice"]      # the planes only behind the span call
    fwd = L.log[6][1]
    assert fwd[5] == P and fwd[6] == out[6].numel() and fwd[9:11] == (0, 2)
    del L.log[:], L.raw[:]
    bf.encode_qa_batch_device(*args, offset_unit="char")                                                          # no answers: on the ragged offsets
    assert names(L) == ["TextToIdsBatchDevice", "TextToIdsWithOffsetsBatchDevice", "ByteToCharOffsetsBatchDevice", "IdsToPairRowsPlanesBatchDevice",
                        "IdsToPairRowsPlanesBatchDevice"]
    with pytest.raises(ValueError):
        bf.encode_qa_batch_device(*args, answer_unit="bytes")
