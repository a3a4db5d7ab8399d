"""GPU: the tokenizer Device calls on batches whose documents lie behind 2^31 bytes of text, and on one whose ids lie behind 2^31 output cells
(tests/big_offset_cases.py has the batches, tests/test_big_offset_cases_host.py holds them to the reference on the CPU).

One pytest test per program, one call per test (batch C: the same call again with a short capacity).  Every test makes its batch on the device
(torch.full for the filler, the real documents copied in behind it), takes a fresh handle, calls BfReserve for the batch's size, runs the call
through the C ABI on torch's stream over canary-filled outputs with a guard of 64 elements behind the capacity, and compares WHOLE arrays: ids,
first and last bytes or strings, and the int64 output offsets of every document equal the checker's, the filler documents are empty (filler B of
a Unigram model: the one id the module states), BfLastStatus is 0, no canary has changed and BfWorkspaceGrows has not moved.

A test is skipped only when the device's free memory is below what big_offset_cases.device_bytes() states for it plus 10 %; on an idle MI355X
none is.  Once a call has failed or the device has reported an error, the tests behind it in this process fail without launching anything.

Cost (MI355X, printed per test): the calls themselves take 0.5 - 33 ms on the device and making the batch a few milliseconds; a test's 0.1 - 6 s
are BfReserve's allocations -- 50 to 200 GB of workspace for a bound of 2 - 4 GiB of text, nothing to a few seconds depending on what the runtime
still holds from the test before -- and, for the Unigram and hyphenation models, 1.3 - 2 s of LoadModel.

Known and left as it is: bf_kernels_sp.hip works out the capacity of a document's arc list and of its right-aligned id slot in `int` from the
document's byte count before it looks at its stream length (k_bpe_collect, k_bpe_collect_list, k_bpe_fused, k_seg_unigram_lane, k_uni_back) --
signed overflow for a document of 2^30 bytes, without effect because the stream of such a document is empty and the number is not used; the
Unigram tests on filler A walk the two Unigram sites."""
import ctypes
import time

import numpy as np
import pytest
import torch

import bfutil
import big_offset_cases as bo
import blingfire_amd as bf

pytestmark = pytest.mark.gpu

vp = ctypes.c_void_p
I32, I64, U8 = torch.int32, torch.int64, torch.uint8
CANARY32, CANARY8, CANARY64 = 0x5A5A5A5A, 0xA5, -0x0123456789ABCDEF
GUARD = bo.GUARD
_broken = []                                                    # the first test whose call failed or whose device reported an error


class launching:
    """around one test's work on the device: a comparison that fails (or a skip) leaves the device as it was; anything else -- a call that answers
    an error, an exception of the runtime -- and the tests behind this one do not launch"""

    def __init__(self, what):
        self.what = what

    def __enter__(self):
        if _broken:
            pytest.fail("not launched: %s failed on the device earlier in this process" % _broken[0])
        _broken.append(self.what)

    def __exit__(self, et, ev, tb):
        if et is None or issubclass(et, (AssertionError, pytest.skip.Exception)):
            _broken.clear()
        return False


def ok(rc, ctx):
    if rc != 0:
        raise RuntimeError("%s: the call answered %d" % (ctx, rc))


class Stages:
    """where a test's wall time goes (printed: the device time of the call itself is milliseconds)"""

    def __init__(self):
        self.t, self.parts = time.perf_counter(), []

    def lap(self, name):
        torch.cuda.synchronize()
        now = time.perf_counter()
        self.parts.append("%s %.2f s" % (name, now - self.t))
        self.t = now

    def __str__(self):
        return ", ".join(self.parts)


def fit(need):
    torch.cuda.empty_cache()
    free = torch.cuda.mem_get_info()[0]
    print("device memory: %.1f GB needed (+ 10 %%), %.1f GB free" % (need / 1e9, free / 1e9))
    if not bo.enough_memory(need, free):
        pytest.skip("%.1f GB of device memory needed (+ 10 %%), %.1f GB free" % (need / 1e9, free / 1e9))


def stream():
    return vp(torch.cuda.current_stream().cuda_stream)


def status(h):
    torch.cuda.synchronize()
    return bf.lib().BfLastStatus(vp(h))


def kernel_name(h):
    L = bf.lib()
    L.BfTokeniseKernel.restype = ctypes.c_char_p
    L.BfTokeniseKernel.argtypes = [vp]
    return L.BfTokeniseKernel(vp(h))


def device_batch(filler, items=None):
    """(text, offsets, documents, bytes, filler documents): the filler made on the device, the items copied in behind it; the 48 bytes behind the batch
    complete the last document's cut character (a kernel that reads past the batch sees a euro sign)"""
    off, nfill = bo.batch_offsets(filler, items)
    total = int(off[-1])
    buf = torch.full((total + 48,), 0xAC, dtype=U8, device="cuda")
    buf[:bo.TWO31].fill_(ord("a") if filler == "A" else 0x20)
    real, _ = bo.pack(bo.real_docs() if items is None else items)
    buf[bo.TWO31:total] = torch.from_numpy(real).cuda()
    return buf[:total], torch.from_numpy(off).cuda(), len(off) - 1, total, nfill


def canary(n, dtype=I32):
    return torch.full((n + GUARD,), {I32: CANARY32, U8: CANARY8, I64: CANARY64}[dtype], dtype=dtype, device="cuda")


def reserve(h, D, B, want_off):
    ok(bf.lib().BfReserve(vp(h), D, B, 1 if want_off else 0), "BfReserve")
    torch.cuda.synchronize()
    return bf.workspace_grows()


def same_arrays(ctx, got_off, want_off, nfill, pairs, fill):
    """whole arrays; on a difference, the first document that differs"""
    assert (got_off[len(want_off):] == CANARY64).all(), ctx + ": written behind the output offsets"
    got_off = got_off[:len(want_off)]
    equal = np.array_equal(got_off, want_off)
    for what, g, w in pairs:
        n = len(w)
        assert (g[n:] == fill).all(), "%s: %s written at or behind the capacity %d" % (ctx, what, n)
        equal = equal and np.array_equal(g[:n], w)
    if equal:
        return
    for d in range(len(want_off) - 1):
        for what, g, w in pairs:
            a, b = g[got_off[d]:got_off[d + 1]], w[want_off[d]:want_off[d + 1]]
            if not np.array_equal(a, b):
                raise AssertionError("%s: document %d (%s): %s gpu (%d) %s != checker (%d) %s" % (
                    ctx, d, "filler" if d < nfill else "real document %d" % (d - nfill), what, len(a), a[:40].tolist(), len(b), b[:40].tolist()))
    raise AssertionError("%s: the output offsets differ: %s != %s" % (ctx, got_off[-3:].tolist(), want_off[-3:].tolist()))


# ------------------------------------------------------------------------------------------------
# TextToIdsBatchDevice / TextToIdsWithOffsetsBatchDevice
# ------------------------------------------------------------------------------------------------
def _run_ids(model, variant, filler, want_off, program=None):
    ctx = "%s variant %s filler %s%s" % (model, variant, filler, " with offsets" if want_off else "")
    fam = bo.family(model)
    per_filler = bo.FILLER_B_IDS[fam] if filler == "B" else 0
    exp = bo.expected_offsets(model) if want_off else bo.expected_ids(model)
    off_np, nfill = bo.batch_offsets(filler)
    D, B = len(off_np) - 1, int(off_np[-1])
    want_id_off = bo.with_filler(exp[-1], nfill, per_filler)
    head = np.full(nfill * per_filler, bo.filler_b_id(model) if per_filler else 0, dtype=np.int32)
    cap = int(want_id_off[-1])
    fit(bo.device_bytes(model, D, B, want_off, variant, out_cells=cap, out_arrays=3 if want_off else 1))
    sw = Stages()
    text, d_off, D, B, nfill = device_batch(filler)
    sw.lap("batch")
    h = bf.load_model(bfutil.model_path(bo.model_file(model)))
    sw.lap("model")
    try:
        L = bf.lib()
        if variant != 3:
            assert L.BfSetVariant(vp(h), variant) == 3          # (answers the variant before: a fresh handle's)
        before = reserve(h, D, B, want_off)
        sw.lap("BfReserve")
        ids, ido = canary(cap), canary(D + 1, I64)
        if want_off:
            st, en = canary(cap), canary(cap)
            rc = L.TextToIdsWithOffsetsBatchDevice(vp(h), text.data_ptr(), d_off.data_ptr(), D, B, ids.data_ptr(), st.data_ptr(), en.data_ptr(), cap, ido.data_ptr(),
                                                   bo.MAX_IDS, bo.UNK[fam], stream())
        else:
            rc = L.TextToIdsBatchDevice(vp(h), text.data_ptr(), d_off.data_ptr(), D, B, ids.data_ptr(), cap, ido.data_ptr(), bo.MAX_IDS, bo.UNK[fam], stream())
        ok(rc, ctx)
        assert status(h) == 0, ctx
        sw.lap("call")
        assert bf.workspace_grows() == before, ctx + ": a workspace grew inside the call"
        if program:
            assert kernel_name(h) == program, (ctx, kernel_name(h))
        ms = bf.last_kernel_ms(h)
        print("%s: %d documents, %d bytes, %d ids, %.2f ms on the device (%s)" % (ctx, D, B, cap, ms[4], ms[5]))
        pairs = [("ids", ids.cpu().numpy(), np.concatenate([head, exp[0]]))]
        if want_off:
            pairs += [("first bytes", st.cpu().numpy(), np.concatenate([head, exp[1]])), ("last bytes", en.cpu().numpy(), np.concatenate([head, exp[2]]))]
        same_arrays(ctx, ido.cpu().numpy(), want_id_off, nfill, pairs, CANARY32)
        assert (want_id_off[:nfill + 1] == np.arange(nfill + 1) * per_filler).all()          # filler A: empty documents
        sw.lap("compare")
    finally:
        bf.free_model(h)
        del text, d_off
        torch.cuda.empty_cache()
        sw.lap("free")
        print("%s: %s" % (ctx, sw))


def run_ids(model, variant, filler, want_off, program=None):
    with launching("%s variant %s filler %s" % (model, variant, filler)):
        _run_ids(model, variant, filler, want_off, program)


# ---- behind 2 GiB of text the kernels skip (filler A: two documents over the reference's limit of 10^9 bytes)
def test_a_bert_wave_program():
    run_ids("bert", 5, "A", False, b"k_wp_wave")


def test_a_bert_lane_kernels():
    run_ids("bert", 2, "A", False)


def test_a_bert_flat_program_hands_every_document_back():
    """documents of 2^30 bytes are more than WF_DOC_MAX: k_wp_pre says `unsafe`, k_wp_flat leaves at once and the wave program takes every document
    from the hand-back list"""
    run_ids("bert", 4, "A", False, b"k_wp_flat")


def test_a_unigram_cut_form():
    run_ids("xlm_roberta_base.bin", 3, "A", False)


def test_a_unigram_lane_form():
    run_ids("xlm_roberta_base.bin", 6, "A", False)


def test_a_xlnet():
    run_ids("xlnet.bin", 3, "A", False)


def test_a_gpt2_bpe_wave_program():
    run_ids("gpt2.bin", 3, "A", False)


def test_a_roberta_bpe_wave_program():
    run_ids("roberta.bin", 3, "A", False)


def test_a_offsets_bert_default():
    run_ids("bert", 3, "A", True, b"k_wp_wave")                 # (two documents of 2^30 bytes and a few hundred small ones: by its own choice the wave program)


def test_a_offsets_bert_lane_kernels():
    run_ids("bert", 2, "A", True)


def test_a_offsets_unigram():
    run_ids("xlm_roberta_base.bin", 3, "A", True)


# ---- behind 2 GiB of text the program walks (filler B: 512 documents of 4 MiB of spaces)
def test_b_bert_flat_program():
    run_ids("bert", 4, "B", False, b"k_wp_flat")


def test_b_bert_flat_program_with_offsets():
    run_ids("bert", 4, "B", True, b"k_wp_flat")


def test_b_bert_wave_program():
    run_ids("bert", 5, "B", False, b"k_wp_wave")


def test_b_unigram_cut_form():
    run_ids("xlm_roberta_base.bin", 3, "B", False)


def test_b_unigram_lane_form():
    run_ids("xlm_roberta_base.bin", 6, "B", False)


# ------------------------------------------------------------------------------------------------
# TextToWordsBatchDevice / TextToSentencesBatchDevice / WordHyphenationBatchDevice on filler A
# ------------------------------------------------------------------------------------------------
def _run_text(what, model_path, fn_name, want, items, u_hy=None):
    ctx = "%s filler A" % what
    w_flat, w_off = want
    off_np, nfill = bo.batch_offsets("A", items)
    D, B = len(off_np) - 1, int(off_np[-1])
    want_off = bo.with_filler(w_off, nfill)
    T = int(want_off[-1])
    fit(bo.device_bytes("bert" if u_hy is None else "w2h", D, B, False, call="text" if u_hy is None else "ids", out_cells=T // 4 + 1))
    sw = Stages()
    text, d_off, D, B, nfill = device_batch("A", items)
    sw.lap("batch")
    h = bf.load_model(model_path)
    sw.lap("model")
    try:
        L = bf.lib()
        before = reserve(h, D, B, False)
        sw.lap("BfReserve")
        out, oo = canary(T, U8), canary(D + 1, I64)
        args = (vp(h), text.data_ptr(), d_off.data_ptr(), D, B, out.data_ptr(), T, oo.data_ptr())
        rc = getattr(L, fn_name)(*args, stream()) if u_hy is None else getattr(L, fn_name)(*args, u_hy, stream())
        ok(rc, ctx)
        assert status(h) == 0, ctx
        sw.lap("call")
        after = bf.workspace_grows()
        assert after[0] - after[1] == before[0] - before[1], ctx + ": a workspace BfReserve sizes grew inside the call"      # (w_long is the call's own: counted apart)
        same_arrays(ctx, oo.cpu().numpy(), want_off, nfill, [("text", out.cpu().numpy(), w_flat)], CANARY8)
        assert (want_off[:nfill + 1] == 0).all()
    finally:
        bf.free_model(h)
        del text, d_off
        torch.cuda.empty_cache()
        sw.lap("free")
        print("%s: %s" % (ctx, sw))


def run_text(what, *args, **kw):
    with launching(what):
        _run_text(what, *args, **kw)


def test_a_text_to_words_built_in_model():
    run_text("TextToWords", bfutil.model_path("wbd.bin"), "TextToWordsBatchDevice", bo.expected_text(1), None)      # models/wbd.bin is the built-in model's file: a handle BfReserve can size


def test_a_text_to_sentences_built_in_model():
    run_text("TextToSentences", bfutil.model_path("sbd.bin"), "TextToSentencesBatchDevice", bo.expected_text(2), None)


def test_a_word_hyphenation():
    """two "words" of 2^30 bytes in front of the words of w2h_cases.edge_words()"""
    import w2h_cases as wc
    run_text("WordHyphenation", wc.FIXTURE, "WordHyphenationBatchDevice", bo.expected_hyphenation(), bo.hyphenation_words(), u_hy=0x2D)


# ------------------------------------------------------------------------------------------------
# batch C: ids beyond 2^31 output cells
# ------------------------------------------------------------------------------------------------
def _run_batch_c(variant, program):
    ctx = "bert variant %d, batch C" % variant
    ck = bo.checker()
    hck = ck.load(bfutil.model_path(bo.model_file("bert")))
    try:
        k, buf = ck.text_to_ids(hck, bo.C_DOC, 512, 100)
    finally:
        ck.free(hck)
    c = bo.batch_c(k)
    N, B, total = c["ndocs"], c["total_bytes"], c["total_ids"]
    fit(bo.device_bytes("bert", N, B, False, variant, out_cells=total) + total + 8 * N)           # (+ the comparisons' byte per id and the expected offsets)
    sw = Stages()
    row = torch.tensor(buf[:k], dtype=I32, device="cuda")
    text = torch.from_numpy(np.frombuffer(bo.C_DOC, dtype=np.uint8).copy()).cuda().repeat(N)
    d_off = torch.arange(N + 1, dtype=I64, device="cuda") * len(bo.C_DOC)
    want_off = torch.arange(N + 1, dtype=I64, device="cuda") * k
    h = bf.load_model(bfutil.model_path(bo.model_file("bert")))
    try:
        L = bf.lib()
        assert L.BfSetVariant(vp(h), variant) == 3              # (answers the variant before: a fresh handle's)
        sw.lap("batch and model")
        before = reserve(h, N, B, False)
        sw.lap("BfReserve")
        ids, ido = canary(total), canary(N + 1, I64)
        s = c["straddler"]

        def call(cap):
            rc = L.TextToIdsBatchDevice(vp(h), text.data_ptr(), d_off.data_ptr(), N, B, ids.data_ptr(), cap, ido.data_ptr(), 512, 100, stream())
            ok(rc, ctx)
            st = status(h)
            assert bf.workspace_grows() == before, ctx + ": a workspace grew inside the call"
            assert kernel_name(h) == program, (ctx, kernel_name(h))
            ms = bf.last_kernel_ms(h)
            print("%s, ids_cap %d: %d documents, %d bytes, %.2f ms on the device (%s)" % (ctx, cap, N, B, ms[4], ms[5]))
            assert bool((ido[:N + 1] == want_off).all()), (ctx, cap, "id offsets")            # complete whatever the capacity
            got_off = torch.cat([ido[:2], ido[s - 1:s + 3], ido[N - 1:]]).cpu().numpy()
            assert got_off.tolist() == [0, k] + [(s - 1 + j) * k for j in range(4)] + [(N - 1) * k, N * k] + [CANARY64] * GUARD, (ctx, cap)
            return st
        # ---- ids_cap = the exact total
        assert call(total) == 0
        assert bool((ids[:total].view(N, k) == row).all()), ctx + ": a document's ids differ from the reference's"
        around = ids[(s - 1) * k:(s + 2) * k].cpu().numpy()     # the documents around output position 2^31, the last one and the guard: copied back
        assert around.tolist() == buf[:k] * 3 and (s * k < bo.TWO31 < (s + 1) * k)
        assert ids[(N - 1) * k:].cpu().numpy().tolist() == buf[:k] + [CANARY32] * GUARD
        # ---- ids_cap = 2^31 + 5: status bit 0, every document wholly below the capacity exact, nothing at or behind it
        cap = bo.TWO31 + 5
        whole, below = bo.batch_c_capped(k, cap)
        ids.fill_(CANARY32); ido.fill_(CANARY64)
        assert call(cap) == 1
        assert bool((ids[:whole * k].view(whole, k) == row).all()), ctx + ": a document below the capacity differs"
        assert bool((ids[cap:] == CANARY32).all()), ctx + ": written at or behind ids_cap"
        cut = ids[whole * k:cap].cpu().numpy().tolist()         # the document the capacity cuts: a prefix of its ids (or nothing)
        assert all(g in (w, CANARY32) for g, w in zip(cut, buf[:k])), (ctx, cut[:8])
        sw.lap("two calls and their comparisons")
    finally:
        bf.free_model(h)
        del text, d_off, want_off
        torch.cuda.empty_cache()
        sw.lap("free")
        print("%s: %s" % (ctx, sw))


def run_batch_c(variant, program):
    with launching("batch C, variant %d" % variant):
        _run_batch_c(variant, program)


def test_c_bert_flat_program_ids_beyond_2_31():
    run_batch_c(4, b"k_wp_flat")


def test_c_bert_wave_program_ids_beyond_2_31():
    run_batch_c(5, b"k_wp_wave")
