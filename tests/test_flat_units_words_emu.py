"""CPU: the word walker of the flat WordPiece program (wf_units, blingfire_amd/csrc/bf_flat_body.h: what k_wp_units runs) in the 64-fibre wave
simulator, through the whole flat program (tests/hosttest bft_emu_flat_batch: wf_units<2, ., 0, .> on the list of the plain words, <1, ., 1, .> and
<1, ., 2, .> on the other list, with and without spans), against the oracle -- on words chosen for the state a lane carries from round to round:
a word of exactly 16 bytes (the last one held in two registers) and of 17; a word whose 16 readable bytes end with the text, and one byte later;
words of 1, 2, 6 and more pieces (the oracle says which they are); words with a character no piece covers (UnkId), short and long; documents
that are nothing but words of several pieces, so that such words of ONE document sit in neighbouring lanes, in lane 63 and lane 0 of the two
words a lane holds, and in the last lane of one batch of 128 and the first of the next (the segmented sum of the ids beyond the entries), with
document boundaries inside a batch.  Whether a word's anchored walk fails before its plain walk succeeds depends on the lexer and is not asserted:
the candidates are walked either way and compared."""
import random

import numpy as np
import pytest

import bfutil
import flat_cases
from test_flat_emu import check, load_hosttest

MODELS = [m for m in ("bert_base_tok.bin", "bert_base_cased_tok.bin", "bert_chinese.bin") if bfutil.have_model(m)]
CONFS = [(512, 100, 1, 1), (512, 100, 2, 3), (16, 7, 1, 0)]          # (max_ids, unk, waves, ranges)


@pytest.fixture(scope="module")
def ht():
    return load_hosttest()


def candidates():
    rnd = random.Random(11)
    words = [bytes(rnd.choice(b"qzxjkvw") for _ in range(n)) for n in range(2, 18) for _ in range(6)]
    words += [bytes(rnd.choice(b"aeinrst") for _ in range(n)) for n in (13, 14, 15, 16, 17) for _ in range(6)]
    words += [w for w in (b"internationally", b"responsibilities", b"characteristics", b"misunderstanding", b"counterproductive", b"unaffable", b"1234567890123456",
                          b"12345678901234567", b"Washingtonians", b"straightforward")]
    return words


def pieces_of(model, words):
    """ids the oracle gives every word as a document of its own"""
    ora = bfutil.oracle()
    ho = ora.load(bfutil.model_path(model))
    text, off = flat_cases.pack(words)
    ids, ido = ora.batch(ho, text, off, 512, 100)
    ora.free(ho)
    return [ids[ido[i]:ido[i + 1]].tolist() for i in range(len(words))]


@pytest.mark.parametrize("model", MODELS)
def test_words_by_length_and_pieces(ht, model):
    words = candidates()
    got = pieces_of(model, words)
    by_n = {}
    for w, ids in zip(words, got):
        by_n.setdefault(len(ids), []).append(w)
    assert any(n >= 7 for n in by_n) and 2 in by_n, sorted(by_n)
    assert any(len(w) == 16 for w in words) and any(len(w) == 17 for w in words)
    # every count the candidates have, two words of it each, in one document; then 16- and 17-byte words side by side
    doc_a = b" ".join(w for n in sorted(by_n) for w in by_n[n][:2])
    doc_b = b" ".join(w for w in words if len(w) in (15, 16, 17))
    # characters no piece covers: in a word of <= 16 bytes (classes made up front) and in a longer one (read from the text)
    doc_c = "ab͸cd qz͸ ͸ abcdefghijklmnop͸qrstu café naïvetés".encode()
    w16 = next(w for w in words if len(w) == 16 and w.isalpha())
    tails = [b"the " + w16, b"the " + w16 + b" ", b"the " + w16[:15], b"a " + next(w for w in words if len(w) == 17)]
    for tail in tails:                                                 # the last word's 16 bytes end with the text, one byte earlier, and it is shorter
        check(ht, model, [doc_a, b"", doc_b, doc_c, tail], CONFS)


@pytest.mark.parametrize("model", MODELS)
def test_words_of_several_pieces_fill_the_lanes(ht, model):
    rnd = random.Random(3)
    word = lambda: bytes(rnd.choice(b"qzxjkvw") for _ in range(rnd.randint(6, 14)))
    docs = [b" ".join(word() for _ in range(n)) for n in (130, 3, 1, 62, 64, 200, 127, 2)]          # boundaries at 130, 133, 134, 196, 260, 460, 587 of the list
    seen = []
    last = check(ht, model, docs, CONFS, want=lambda st: seen.append(int(st[4])))
    assert last is not None and min(seen) >= 500                       # (the words went to the walker, not to the table)
