"""GPU parity of the flat WordPiece program where the number of its ranges is decided (wp_flat_ranges, bf_kernels.hip): the ranges follow the waves
that are resident, cut down so that a range keeps 16 KB, and never more than there are documents.  TextToIdsBatch against the CPU checker (the
compiled reference where oracle/_ref is built, else the oracle), ids and id offsets of every document, bit for bit.

  most    2,052 documents of exactly 600 bytes (just over use_flat's threshold of 1,024 documents / 1 MiB) plus empty ones: 1,231,200 bytes are 76
          ranges of 16,200 bytes = 27 documents, so EVERY range boundary is the first byte of a document, and some of those documents are empty
  ndocs   twelve documents of 20,000 bytes: fifteen ranges of 16 KB would fit, twelve documents allow twelve (BfSetVariant 4: the flat program for
          a batch under the threshold)
The third bound (a range of at most WF_RANGE_MAX = 4 MiB) binds only when sixteen ranges per resident wave are each longer than that: hundreds of
gigabytes in one batch, more than the device holds, so no test can reach it."""
import ctypes

import numpy as np
import pytest

import bfutil
import blingfire_amd as bf
import flat_cases

pytestmark = pytest.mark.gpu

MODEL = "bert_base_tok.bin" if bfutil.have_model("bert_base_tok.bin") else "bert_base_cased_tok.bin"
DOC_BYTES, NDOCS, NRANGES = 600, 2052, 76                 # 2,052 * 600 // 16,384 + 1 = 76 ranges of 27 documents
PER_RANGE = NDOCS // NRANGES
EMPTY_AT = (0, PER_RANGE, PER_RANGE, 5 * PER_RANGE, 5 * PER_RANGE + 1, 1000, NDOCS - 1, NDOCS)      # (before these documents of the plain batch)

_made = {}


def body():
    """headline documents with words no vocabulary holds between them (words of several pieces for k_wp_units), as one run of bytes"""
    if "body" not in _made:
        head, odd = flat_cases.headline(2600), flat_cases.many_docs(24)
        _made["body"] = b" ".join(d + b" " + odd[i % len(odd)][:40 + i % 50] for i, d in enumerate(head))
    return _made["body"]


def batch_most():
    if "most" not in _made:
        raw = body()
        assert len(raw) >= NDOCS * DOC_BYTES
        docs = [raw[i * DOC_BYTES:(i + 1) * DOC_BYTES] for i in range(NDOCS)]
        for at in sorted(EMPTY_AT, reverse=True):
            docs.insert(at, b"")
        text, off = flat_cases.pack(docs)
        text.flags.writeable = False; off.flags.writeable = False
        _made["most"] = (text, off)
    return _made["most"]


def batch_ndocs():
    if "ndocs" not in _made:
        raw = body()
        text, off = flat_cases.pack([raw[i * 20000:(i + 1) * 20000] for i in range(12)])
        text.flags.writeable = False; off.flags.writeable = False
        _made["ndocs"] = (text, off)
    return _made["ndocs"]


@pytest.fixture(scope="module")
def checker():
    ck = bfutil.reference() if bfutil.have_ref() else bfutil.oracle()
    hck = ck.load(bfutil.model_path(MODEL))
    yield ck, hck
    ck.free(hck)


def flat_ran(h):
    L = bf.lib()
    L.BfTokeniseKernel.restype = ctypes.c_char_p
    L.BfTokeniseKernel.argtypes = [ctypes.c_void_p]
    assert L.BfTokeniseKernel(ctypes.c_void_p(h)) == b"k_wp_flat"
    assert L.BfLastStatus(ctypes.c_void_p(h)) == 0


def compare(batch, got, want, what):
    (ids, id_off), (wids, woff) = got, want
    if np.array_equal(id_off, woff) and np.array_equal(ids, wids):
        return
    text, off = batch
    for d in range(len(off) - 1):
        a, b = ids[id_off[d]:id_off[d + 1]], wids[woff[d]:woff[d + 1]]
        assert np.array_equal(a, b), (what, d, bytes(text[off[d]:off[d + 1]][:80]), a[:24].tolist(), b[:24].tolist())
    raise AssertionError("%s: the id offsets differ behind the last document" % what)


def test_the_batches_are_what_the_bounds_need():
    text, off = batch_most()
    nd = len(off) - 1
    assert nd >= 1024 and len(text) >= 1 << 20 and len(text) == NDOCS * DOC_BYTES
    assert len(text) // 16384 + 1 == NRANGES and len(text) % NRANGES == 0
    starts = set(off[:-1].tolist())
    assert all(len(text) * r // NRANGES in starts for r in range(NRANGES))                 # every range begins with a document's first byte
    sizes = np.diff(off)
    assert (sizes == 0).sum() == len(EMPTY_AT) and sizes[0] == 0 and sizes[-1] == 0
    first_of = np.searchsorted(off[:-1], [len(text) * r // NRANGES for r in (1, 5)])         # the first document at a boundary is an empty one
    assert (sizes[first_of] == 0).all()
    text, off = batch_ndocs()
    assert len(off) - 1 == 12 < len(text) // 16384 + 1


@pytest.mark.parametrize("max_ids", [512, 16])
def test_just_over_the_threshold_every_range_begins_a_document(checker, max_ids):
    ck, hck = checker
    batch = batch_most()
    want = ck.batch(hck, batch[0], batch[1], max_ids, 100)
    h = bf.load_model(bfutil.model_path(MODEL))
    try:
        got = bf.text_to_ids_batch(h, batch, max_ids, 100)
        flat_ran(h)
        compare(batch, got, want, "max_ids %d" % max_ids)
        again = bf.text_to_ids_batch(h, batch, max_ids, 100)                              # the workspaces of the first call, reused
        assert again[0].tobytes() == got[0].tobytes() and again[1].tobytes() == got[1].tobytes()
    finally:
        bf.free_model(h)


@pytest.mark.parametrize("max_ids", [512, 16])
def test_as_many_ranges_as_documents(checker, max_ids):
    ck, hck = checker
    batch = batch_ndocs()
    want = ck.batch(hck, batch[0], batch[1], max_ids, 100)
    h = bf.load_model(bfutil.model_path(MODEL))
    try:
        bf.lib().BfSetVariant(h, 4)
        got = bf.text_to_ids_batch(h, batch, max_ids, 100)
        flat_ran(h)
        compare(batch, got, want, "max_ids %d" % max_ids)
    finally:
        bf.free_model(h)
