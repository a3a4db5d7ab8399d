"""One handle, one small batch, every program run_device can dispatch to, in an order that makes each program follow another one: what is
checked is what a program can inherit from the program before it -- a control word of the handle's device control block
that nobody cleared, or a timing event the program did not record.  The calls are the Device ones on torch tensors; every id, id offset,
start and end of every document is compared with the CPU checker (the compiled reference where oracle/_ref is built, else the oracle)."""
import ctypes
import math

import pytest

import bfutil
import blingfire_amd as bf

pytestmark = pytest.mark.gpu

# about 600 bytes.  "[" and a run of more than 48 bytes without a break make the flat program hand a document back to the wave program
# (its unsafe / list_n words and its own compaction of the handed-back documents)
DOCS = [
    b"",
    b"hello",
    "Zürich naïve café, 東京の朝 and Привет — 😀 𝒳 ok".encode(),
    b"What makes working with natural language so challenging. [1] See the notes below.",
    b"fetch https://example.org/abcdefghijklmnopqrstuvwxyz0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZ0123 and report back",
    (b"After reading this post, you will know: what natural language is and how it is different from other types of data; "
     b"what makes working with it so challenging, and where the field of unaffable telescopes came from. Hello, world! This is a test "
     b"of 3,000.50 e-mails that don't reach the U.S.A. in time."),
]
MAX_IDS = 512

WP = (bfutil.bert_model_name(), 100, (4, 5, 2, 4, 5, 4))          # the flat program, the wave program, the lane lexer (tests/test_gpu_parity_wp.py)
UNIGRAM = ("xlnet.bin", 0, (3, 6, 3))                              # the cut form, the lane form (tests/test_gpu_parity_sp.py)
BPE = ("gpt2.bin", 0, (3, 3 | 0x40, 3))                            # the BPE wave program, the lane kernels alone
# what BfTokeniseKernel answers behind an ids-only batch of each (model, variant): the call took the program it was meant to take
KERNEL = {(WP[0], 4): (b"k_wp_flat",), (WP[0], 5): (b"k_wp_wave",), (WP[0], 2): (b"k_lex_wp_plain", b"k_lex_wp_flat"),
          (UNIGRAM[0], 3): (b"k_uni_cut",), (UNIGRAM[0], 6): (b"k_seg_unigram_lane",), (BPE[0], 3): (b"k_bpe_wave",), (BPE[0], 3 | 0x40): (b"k_bpe_fused",)}


def expected(model, unk):
    """per document (ids, starts, ends) of the checker's TextToIds and TextToIdsWithOffsets; both must answer every document"""
    ref = bfutil.have_ref()
    ck = bfutil.reference() if ref else bfutil.oracle()
    name = "TextToIdsWithOffsets" if ref else "bfo_text_to_ids_with_offsets"
    hck = ck.load(bfutil.model_path(model))
    try:
        text, off = bf.pack_docs(DOCS)
        ids, id_off = ck.batch(hck, text, off, MAX_IDS, unk)
        out = []
        for d, b in enumerate(DOCS):
            c, wi, ws, we = ck.with_offsets(hck, b, MAX_IDS, unk, name)
            plain = [int(x) for x in ids[id_off[d]:id_off[d + 1]]]
            assert 0 <= c < MAX_IDS and list(wi) == plain, (model, d)       # the two calls agree, nothing was cut
            assert (c > 0) == (d > 0), (model, d)                               # only the empty document is empty
            out.append((plain, list(ws), list(we)))
        return out
    finally:
        ck.free(hck)


class Batch:
    def __init__(self, docs):
        import torch
        text, off = bf.pack_docs(docs)
        self.n, self.total = len(docs), int(off[-1])
        self.d_text = torch.from_numpy(text.copy()).cuda()
        self.d_off = torch.from_numpy(off).cuda()
        self.stream = torch.cuda.current_stream().cuda_stream


def check_launch(h, nonempty, what):
    L = bf.lib()
    assert L.BfLastStatus(ctypes.c_void_p(h)) == 0, what
    ms = bf.last_kernel_ms(h)
    print(what, "ms", [round(float(v), 4) for v in ms])
    assert len(ms) == 6 and all(math.isfinite(v) and v >= 0 for v in ms), (what, ms)
    assert ms[5] <= ms[1] <= ms[4], (what, ms)
    if nonempty:
        assert ms[5] > 0, (what, ms)


def run_ids(h, b, unk, want, what):
    import torch
    ids, id_off = bf.text_to_ids_batch_device(h, b.d_text, b.d_off, MAX_IDS, unk)
    torch.cuda.synchronize()
    o = id_off.cpu().numpy()
    got = ids[:int(o[-1])].cpu().numpy()
    assert o[0] == 0 and [[int(x) for x in got[o[d]:o[d + 1]]] for d in range(b.n)] == [w[0] for w in want], what
    check_launch(h, b.n > 0, what)


def run_offsets(h, b, unk, want, what):
    import torch
    cap = max(1, b.n * MAX_IDS)
    ids, st, en = (torch.full((cap,), -7, dtype=torch.int32, device="cuda") for _ in range(3))
    id_off = torch.empty(b.n + 1, dtype=torch.int64, device="cuda")
    r = bf.lib().TextToIdsWithOffsetsBatchDevice(ctypes.c_void_p(h), b.d_text.data_ptr(), b.d_off.data_ptr(), b.n, b.total, ids.data_ptr(), st.data_ptr(),
                                                 en.data_ptr(), cap, id_off.data_ptr(), MAX_IDS, unk, ctypes.c_void_p(b.stream))
    assert r == 0, what
    torch.cuda.synchronize()
    o = id_off.cpu().numpy()
    assert o[0] == 0
    for k, t in enumerate((ids, st, en)):
        a = t[:int(o[-1])].cpu().numpy()
        assert [[int(x) for x in a[o[d]:o[d + 1]]] for d in range(b.n)] == [w[k] for w in want], (what, ("ids", "starts", "ends")[k])
    check_launch(h, b.n > 0, what + " with offsets")


def run_programs(model, unk, variants, offsets_each_time):
    want = expected(model, unk)
    batch, empty = Batch(DOCS), Batch([])
    h = bf.load_model(bfutil.model_path(model))
    L = bf.lib()
    L.BfTokeniseKernel.restype = ctypes.c_char_p; L.BfTokeniseKernel.argtypes = [ctypes.c_void_p]
    try:
        for k, v in enumerate(variants):
            assert bf.lib().BfSetVariant(ctypes.c_void_p(h), v) >= 0
            what = "%s call %d variant 0x%x" % (model, k, v)
            run_ids(h, batch, unk, want, what)
            assert L.BfTokeniseKernel(ctypes.c_void_p(h)) in KERNEL[(model, v)], what
            if offsets_each_time:
                run_offsets(h, batch, unk, want, what)
        if not offsets_each_time:
            run_offsets(h, batch, unk, want, "%s variant 0x%x" % (model, variants[-1]))
        run_ids(h, empty, unk, [], "%s no documents" % model)
        run_offsets(h, empty, unk, [], "%s no documents" % model)
        run_ids(h, batch, unk, want, "%s behind the empty batch" % model)
    finally:
        bf.free_model(h)


def test_wordpiece_flat_wave_lane_on_one_handle():
    run_programs(*WP, offsets_each_time=True)


def test_unigram_cut_and_lane_form_on_one_handle():
    run_programs(*UNIGRAM, offsets_each_time=False)


def test_bpe_wave_and_lane_kernels_on_one_handle():
    run_programs(*BPE, offsets_each_time=False)


@pytest.mark.parametrize("mode", [1, 2])
def test_words_and_sentences_on_the_default_handles(mode):
    """TextToWordsBatchDevice / TextToSentencesBatchDevice on the built-in models (the lane lexer in its words / sentences mode), twice in a row"""
    import torch
    ask, close = bfutil.words_checker(None, mode)
    try:
        want = []
        for b in DOCS:
            r, o, _, _ = ask(b, 4 * len(b) + 8)
            want.append(o[:r - 1] if r > 0 else b"")
        assert all((len(w) > 0) == (len(b) > 0) for w, b in zip(want, DOCS))
        fn = bf.lib().TextToWordsBatchDevice if mode == 1 else bf.lib().TextToSentencesBatchDevice
        b = Batch(DOCS)
        for _ in range(2):
            cap = 4 * b.total + 8 * b.n
            out = torch.full((cap,), 0x7f, dtype=torch.uint8, device="cuda")
            t_off = torch.empty(b.n + 1, dtype=torch.int64, device="cuda")
            assert fn(None, b.d_text.data_ptr(), b.d_off.data_ptr(), b.n, b.total, out.data_ptr(), cap, t_off.data_ptr(), ctypes.c_void_p(b.stream)) == 0
            torch.cuda.synchronize()
            o = t_off.cpu().numpy()
            raw = out[:int(o[-1])].cpu().numpy().tobytes()
            assert o[0] == 0 and [raw[o[d]:o[d + 1]] for d in range(b.n)] == want
    finally:
        close()
