"""The offsets calls of the BPE models on the wave program: the SPANS instance of k_bpe_wave (an id under its piece's first element) -> scan ->
k_bpe_home_spans.  One table of small batches, each the smallest at which the new code can go wrong; every id, first byte, last
byte and id offset of TextToIdsWithOffsetsBatchDevice against the checker called one document at a time (the compiled reference where
oracle/_ref is built, else the oracle), with ids_cap = the total and one short of it in canary-filled arrays, and the same batch under
BfSetVariant 3 | 0x40 (the lane kernels and k_compact) for equal outputs.  A stream element of these documents is one byte behind the dummy
prefix, so the cell of a token is its first byte + 1: the block-edge property of a case is asserted from the checker's offsets first."""
import ctypes

import numpy as np
import pytest

import bfutil

bf = pytest.importorskip("blingfire_amd")
pytestmark = pytest.mark.gpu

MODELS = [m for m in ("gpt2.bin", "roberta.bin", "bpe_example.bin", "bpe_example2.bin") if bfutil.have_model(m)]
UNK, TAIL = 0, 64
ODD = b"bc" + b" a" * 100          # "_bc" in cells 0..2, then a two-element word "_a" in every odd cell: 63 | 65, 127 | 129, 191 | 193
EVEN = b"bcd" + b" a" * 100        # ... in every even cell: a piece ends in the last cell of a block
Q = b"qxzjvk" * 11                 # every letter a piece of its own
# case -> (documents, max_ids, (a document, cells of it that must start a token: the last cell of a block of 64, the next token in the next block or none))
CASES = {
    "entry_and_split": ([b"the", b"unaffable", b"----------------", b"x"], 64, (0,)),                 # the word table, two pieces, a word a unit takes whole
    "small_big_huge": ([Q[:61], b"a" * 20, b"a" * 40, b"pneumonoultramicroscopic"], 64, (0,)),        # unit_solve_small (62 elements), solve_big, unit_huge
    "word_63_handed_back": ([b"the cat", b"in " + Q[:62] + b" out", b"sat"], 128, (0,)),             # between two documents that are not
    "blocks_63_64_65": ([ODD[:62], EVEN[:63], ODD[:64]], 128, (2, 63)),
    "blocks_127_128_129": ([ODD[:126], EVEN[:127], ODD[:128]], 128, (2, 63, 127)),
    "blocks_193": ([ODD[:192], Q[:61] + b" " + Q[:61] + b" " + Q[:61]], 256, (0, 63, 127, 191)),       # across the 128-cell trip, and ends from the look-ahead mask
    "max_ids_1": ([ODD[:66]], 1, (0, 63)),                                                           # 33 tokens, the last one in cell 65
    "max_ids_count_less_1": ([ODD[:66]], 32, (0, 63)),                                               # the end of the last kept token comes from the dropped one's cell
    "max_ids_count": ([ODD[:66]], 33, (0, 63)),
    "multibyte": (["é 日本 😀😀 ª".encode(), "naïve 😀".encode(), "日".encode()], 64, (0,)),             # bytes of one character in different tokens
    "empty_and_blank": ([b"", b" ", b"   ", b"a", b"", b"ends with x"], 64, (0,)),
}


@pytest.fixture(scope="module")
def checker():
    return (bfutil.reference(), "TextToIdsWithOffsets") if bfutil.have_ref() else (bfutil.oracle(), "bfo_text_to_ids_with_offsets")


def device_call(h, docs, max_ids, cap):
    """TextToIdsWithOffsetsBatchDevice into arrays of cap + TAIL canaries -> ids, starts, ends, id offsets, status"""
    import torch
    text, off = bf.pack_docs(docs)
    dt = torch.from_numpy(text.copy()).cuda() if len(text) else torch.zeros(1, dtype=torch.uint8, device="cuda")
    do = torch.from_numpy(off).cuda()
    outs = [torch.full((cap + TAIL,), -7, dtype=torch.int32, device="cuda") for _ in range(3)]
    ido = torch.full((len(docs) + 1,), -7, dtype=torch.int64, device="cuda")
    L = bf.lib()
    r = L.TextToIdsWithOffsetsBatchDevice(ctypes.c_void_p(h), dt.data_ptr(), do.data_ptr(), len(docs), len(text), outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(),
                                          cap, ido.data_ptr(), max_ids, UNK, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert r == 0
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in outs] + [ido.cpu().numpy(), L.BfLastStatus(ctypes.c_void_p(h))]


def lex_stats(h):
    st = (ctypes.c_ulonglong * 16)()
    bf.lib().BfLexStats(ctypes.c_void_p(h), st, 16)
    return list(st)


@pytest.mark.parametrize("case", sorted(CASES))
@pytest.mark.parametrize("model", MODELS)
def test_offsets_on_the_wave_program(model, case, checker):
    docs, max_ids, (edge_doc, *edges) = CASES[case]
    ck, name = checker
    hck = ck.load(bfutil.model_path(model))
    rows = [ck.with_offsets(hck, d, max_ids, UNK, name) for d in docs]
    full = ck.with_offsets(hck, docs[edge_doc], 4096, UNK, name)
    ck.free(hck)
    cells = [s + 1 for s in full[2]]
    assert all(e in cells and (e + 1) % 64 == 0 for e in edges) and (not full[0] or full[3][-1] == len(docs[edge_doc]) - 1), (model, case, cells)      # (the last piece ends at L - 1)
    cat = lambda k: np.array([x for r in rows for x in r[k]], dtype=np.int32)
    wi, ws, we, woff = cat(1), cat(2), cat(3), np.concatenate([[0], np.cumsum([r[0] for r in rows])]).astype(np.int64)
    n = int(woff[-1])
    L = bf.lib()
    h = bf.load_model(bfutil.model_path(model))
    try:
        L.BfSetLexStats(ctypes.c_void_p(h), 1)
        for cap in (n, n - 1):
            gi, gs, ge, goff, status = device_call(h, docs, max_ids, cap)
            assert np.array_equal(goff, woff), (model, case, cap)
            for what, g, w in (("ids", gi, wi), ("starts", gs, ws), ("ends", ge, we)):
                assert np.array_equal(g[:cap], w[:cap]) and (g[cap:] == -7).all(), (model, case, cap, what, g[:cap].tolist(), w[:cap].tolist())
            assert (status & 1) == (1 if cap < n else 0), (model, case, cap, status)
        st = lex_stats(h)
        assert st[0] + st[12] > 0, (model, case, "no word went through k_bpe_wave", st)
        if model == "gpt2.bin":
            want = {"entry_and_split": (12, 1), "small_big_huge": (8, 11, 7), "word_63_handed_back": (3,)}.get(case, ())
            assert all(st[k] > 0 for k in want), (case, st)
        L.BfSetVariant(ctypes.c_void_p(h), 3 | 0x40)
        L.BfSetLexStats(ctypes.c_void_p(h), 1)
        vi, vs, ve, voff, _ = device_call(h, docs, max_ids, n)
        assert np.array_equal(voff, woff) and np.array_equal(vi[:n], wi) and np.array_equal(vs[:n], ws) and np.array_equal(ve[:n], we), (model, case, "variant 3 | 0x40")
        st = lex_stats(h)
        assert st[0] == 0 and st[12] == 0, (model, case, "the lane kernels count no words", st)
    finally:
        bf.free_model(h)


@pytest.mark.skipif("gpt2.bin" not in MODELS, reason="gpt2.bin not present")
def test_ordinary_lines_take_the_wave_program():
    """an offsets call on a few hundred ordinary lines: words seen by k_bpe_wave (BfLexStats slot 0) and words its table answered (slot 12);
    under 3 | 0x40 neither"""
    text, off = bfutil.gen_workload("config3", 300)
    docs = [bytes(text[off[d]:off[d + 1]]) for d in range(len(off) - 1)]
    L = bf.lib()
    h = bf.load_model(bfutil.model_path("gpt2.bin"))
    try:
        seen = {}
        for variant in (3, 3 | 0x40):
            L.BfSetVariant(ctypes.c_void_p(h), variant)
            L.BfSetLexStats(ctypes.c_void_p(h), 1)
            seen[variant] = device_call(h, docs, 512, len(text) + len(docs))[:4], lex_stats(h)
        assert seen[3][1][0] > 0 and seen[3][1][12] > 0 and seen[3 | 0x40][1][0] == 0 and seen[3 | 0x40][1][12] == 0, (seen[3][1], seen[3 | 0x40][1])
        for a, b in zip(seen[3][0], seen[3 | 0x40][0]):
            assert np.array_equal(a, b)
    finally:
        bf.free_model(h)
