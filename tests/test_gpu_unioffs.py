"""The offsets calls of the Unigram models on the cut form: k_uni_cut's spans instance -> scan -> k_uni_ids' offsets instance.
One table of small batches, each the smallest at which the span words can go wrong; every id, first byte, last byte and id offset against
the checker (the compiled reference where oracle/_ref is built, else the oracle), the outputs in canary-filled arrays, BfTokeniseKernel ==
k_uni_cut after every call, and the same batch under BfSetVariant 6 (the forward / backward kernels and k_compact) for equal outputs."""
import ctypes

import numpy as np
import pytest

import bfutil

bf = pytest.importorskip("blingfire_amd")
pytestmark = pytest.mark.gpu

MODELS = [m for m in ("xlm_roberta_base.bin", "xlnet.bin", "laser500k.bin") if bfutil.have_model(m)]
UNK, TAIL = 3, 64
PUA = "\U000F0000"                                                    # outside every vocabulary
THAI, CJK = "การทดสอบภาษาไทย" * 20, "日本語のテキスト中文字符" * 25        # no blanks, about 300 characters each
LINE = "Hello, world! ﬁne café ª test"
ONE = ["a", "the", "of", "I"]
# (documents, max_ids, no dummy prefix)
CASES = {
    "minimal": (["", " ", "a", "\U0001F600"], 64, False),                                     # from == to; the end covers the whole last character
    "charmap": (["ª ﬁ ㍿", "xﬁy wordª", "a㍿", "ﬁ"], 64, False),                               # several stream elements from one source character
    "long_and_unknown": (["pneumonoultramicroscopicsilicovolcanoconi next", "hello " + PUA + " world", "a " + PUA * 200 + " b"], 512, False),   # the ring spills; runs of 1 and > UC_RUN_MAX
    "no_blanks": ([THAI, CJK, THAI[7:] + CJK], 1024, False),                                  # cuts wherever the arcs allow; > 128 walked words: the LDS list wraps
    "dummy_on": ([LINE, " " + LINE, "a"], 64, False),
    "dummy_off": ([LINE, " " + LINE, "a"], 64, True),
    "docs_65": ([ONE[k % 4] + " " + str(k) for k in range(65)], 64, False),                   # document 64 goes to the next wave of k_uni_ids
    "docs_129": ([LINE if k % 9 == 0 else ONE[k % 4] for k in range(129)], 64, False),
    "one_long_among_short": (ONE * 5 + [LINE * 8] + ONE * 5, 1024, False),                    # more than 64 tokens among one-token documents
    "truncated": ([LINE * 3, THAI, "a", LINE], 5, False),                                     # max_ids below the token count
}


@pytest.fixture(scope="module")
def checker():
    ck, name = (bfutil.reference(), "TextToIdsWithOffsets") if bfutil.have_ref() else (bfutil.oracle(), "bfo_text_to_ids_with_offsets")
    setter = getattr(ck.lib, "SetNoDummyPrefix", None) or getattr(ck.lib, "bfo_set_no_dummy_prefix")
    setter.argtypes = [ctypes.c_void_p, ctypes.c_int]
    return ck, name, setter


def answers(checker, model, docs, max_ids, nodummy):
    ck, name, setter = checker
    hck = ck.load(bfutil.model_path(model))
    try:
        setter(ctypes.c_void_p(hck), int(nodummy))
        rows = [ck.with_offsets(hck, d.encode("utf-8"), max_ids, UNK, name) for d in docs]
    finally:
        ck.free(hck)
    cat = lambda k: np.array([x for r in rows for x in r[k]], dtype=np.int32)
    return cat(1), cat(2), cat(3), np.concatenate([[0], np.cumsum([r[0] for r in rows])]).astype(np.int64)


def device_call(h, docs, max_ids, cap):
    """TextToIdsWithOffsetsBatchDevice into arrays of cap + TAIL canaries -> (ids, starts, ends, id offsets, status); the kernel must be the cut form's unless variant 6 is set"""
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
    L.BfTokeniseKernel.restype = ctypes.c_char_p; L.BfTokeniseKernel.argtypes = [ctypes.c_void_p]
    return [t.cpu().numpy() for t in outs] + [ido.cpu().numpy(), L.BfLastStatus(ctypes.c_void_p(h)), L.BfTokeniseKernel(ctypes.c_void_p(h))]


@pytest.mark.parametrize("case", sorted(CASES))
@pytest.mark.parametrize("model", MODELS)
def test_offsets_on_the_cut_form(model, case, checker):
    docs, max_ids, nodummy = CASES[case]
    wi, ws, we, woff = answers(checker, model, docs, max_ids, nodummy)
    n = int(woff[-1])
    h = bf.load_model(bfutil.model_path(model))
    try:
        bf.change_settings_dummy_prefix(h, not nodummy)
        # the whole batch; ids_cap inside the last document with ids, and exactly at the boundary in front of it
        last = max(d for d in range(len(docs)) if woff[d + 1] > woff[d])
        caps = [n, int(woff[last]) + (int(woff[last + 1] - woff[last]) + 1) // 2, int(woff[last])]
        for cap in caps:
            gi, gs, ge, goff, status, kernel = device_call(h, docs, max_ids, cap)
            assert kernel == b"k_uni_cut", (model, case, cap, kernel)
            assert np.array_equal(goff, woff), (model, case, cap)
            m = n if cap == n else int(woff[last])                     # the documents wholly below the cap
            for name, g, w in (("ids", gi, wi), ("starts", gs, ws), ("ends", ge, we)):
                assert np.array_equal(g[:m], w[:m]), (model, case, cap, name, g[:m].tolist(), w[:m].tolist())
                assert np.array_equal(g[m:min(cap, n)], w[m:min(cap, n)]) and (g[cap:] == -7).all(), (model, case, cap, name, "at or past the cap")
            assert (status & 1) == (1 if cap < n else 0), (model, case, cap, status)
        bf.lib().BfSetVariant(ctypes.c_void_p(h), 6)
        vi, vs, ve, voff, _, kernel = device_call(h, docs, max_ids, n)
        assert kernel == b"k_seg_unigram_lane"
        assert np.array_equal(voff, woff) and np.array_equal(vi[:n], wi) and np.array_equal(vs[:n], ws) and np.array_equal(ve[:n], we), (model, case, "variant 6")
    finally:
        bf.free_model(h)


@pytest.mark.skipif("xlm_roberta_base.bin" not in MODELS, reason="xlm_roberta_base.bin not present")
def test_wrapper_chain_equals_variant_6():
    """encode_batch_device(..., return_offsets=True, offset_unit="char") on the cut form against the same chain on the forward / backward kernels"""
    import torch
    text, off = bf.pack_docs(CASES["charmap"][0] + CASES["no_blanks"][0] + [LINE * 4, ""])
    dt, do = torch.from_numpy(text.copy()).cuda(), torch.from_numpy(off).cuda()
    L = bf.lib()
    L.BfTokeniseKernel.restype = ctypes.c_char_p; L.BfTokeniseKernel.argtypes = [ctypes.c_void_p]
    h = bf.load_model(bfutil.model_path("xlm_roberta_base.bin"))
    try:
        got = {}
        for variant, kernel in ((3, b"k_uni_cut"), (6, b"k_seg_unigram_lane")):
            L.BfSetVariant(ctypes.c_void_p(h), variant)
            out = bf.encode_batch_device(h, dt, do, 48, 0, 2, 1, unk=UNK, stride=8, max_rows_per_doc=0, return_offsets=True, offset_unit="char")
            torch.cuda.synchronize()
            assert L.BfTokeniseKernel(ctypes.c_void_p(h)) == kernel
            got[variant] = [t.cpu().numpy() for t in out]
        assert len(got[3]) == 6 and got[3][0].shape[0] > len(off) - 1
        for a, b in zip(got[3], got[6]):
            assert np.array_equal(a, b)
    finally:
        bf.free_model(h)
