"""TEST helpers of the BfReserve contract (tests/test_gpu_reserve_contract.py, GPU tier; tests/test_reserve_cases_host.py, CPU tier): batches
for a bound (D documents, B bytes) that lie within the bound and, where they say so, touch it exactly -- a workspace that BfReserve sized a
little too small then has to grow inside the call, and the allocation counter (BfWorkspaceGrows) sees it.

    even       D documents, B bytes in all, about B / D bytes each
    one_long   D - 1 empty documents and one of B bytes, made of one- and two-letter words: more than 2048 bytes (k_prep_wp_long), more than
               1024 tokens (k_w2t_copy_long), longer than the long-document threshold of the words modes for this B (long_threshold below)
    bytes      min(D, B) documents of one byte
    expanding  (models with a 1 : n charmap) D documents of characters whose normalisation has more elements than the character has bytes
    empty      no documents
    half       `even` at D / 2, B / 2

The first three touch the bound (`bytes` in its documents alone), `expanding` touches it too; a batch is filled to exactly D documents and B bytes
by trimming or padding its last document.  The sequence shapes (seq_shapes) are the same idea for the calls whose D counts id sequences or keys."""
import unicodedata

import numpy as np

import bfutil

SMALL = (64, 8 << 10)                       # every program a BfSetVariant value can force on a small batch
BY_SIZE = (1100, (6 << 20) // 5)            # 1.2 MiB: past use_flat's size test (>= 1024 documents and >= 1 MiB), the flat program by the library's own choice
TOUCHING = ("even", "one_long", "expanding")   # D documents and B bytes exactly
SHORT_WORDS = [b"a", b"is", b"I", b"of", b"x", b"to", b"b", b"we", b"c", b"it", b"no", b"d", b"up", b"e", b"so"]


def long_threshold(B):
    """the words modes list a document as long from this many characters on (bf_capi.cpp long_caps: B / 24,000, at least 16)"""
    return max(16, B // 24000)


def _words_text(n, seed):
    """exactly n bytes of English words (tests/data/words_en.txt) with single spaces between them, cut where n falls"""
    ws = open(bfutil.WORDS_EN).read().split()
    rnd = np.random.RandomState(seed)
    out, size = [], 0
    while size < n + 1:
        w = ws[int(rnd.randint(0, len(ws)))]
        out.append(w)
        size += len(w) + 1
    return " ".join(out).encode()[:n]


def even(D, B, seed=1):
    text = _words_text(B, seed)
    cuts = [B * i // D for i in range(D + 1)]
    return [text[cuts[i]:cuts[i + 1]] for i in range(D)]


def one_long(D, B):
    reps = B // sum(len(w) + 1 for w in SHORT_WORDS) + 1
    doc = b" ".join(SHORT_WORDS * reps)[:B]
    docs = [b""] * D
    docs[D // 2] = doc
    return docs


def one_byte(D, B):
    alphabet = b"a. b,Z\n9-"
    return [alphabet[i % len(alphabet):i % len(alphabet) + 1] for i in range(min(D, B))]


def expanding_chars(pieces="xlmr"):
    """the characters of the `charmap` lines of tests/data/pieces_<name>.tsv.gz whose compatibility decomposition has more code points than the
    character has UTF-8 bytes (the models' charmaps are NFKC tables; the CPU test counts the elements with the model's own charmap)"""
    cm_blob, cm_off = bfutil._pieces(pieces)[5:7]
    raw = cm_blob.tobytes()
    chars = [raw[cm_off[i]:cm_off[i + 1]] for i in range(len(cm_off) - 1)]
    return [c for c in chars if len(unicodedata.normalize("NFKC", c.decode("utf-8"))) > len(c)]


def expanding(D, B, pieces="xlmr"):
    chars = expanding_chars(pieces)
    assert chars
    cuts = [B * i // D for i in range(D + 1)]
    docs, k = [], 0
    for i in range(D):
        want, parts, size = cuts[i + 1] - cuts[i], [], 0
        while size + len(chars[k % len(chars)]) <= want:
            parts.append(chars[k % len(chars)])
            size += len(parts[-1])
            k += 1
        docs.append(b"".join(parts) + b"a" * (want - size))      # (a character that does not fit any more: the document is padded to its share)
    return docs


def shapes(D, B, pieces=None):
    """name -> list of documents, in the order the tests call them: the shapes that touch the bound come first"""
    out = {"even": even(D, B), "one_long": one_long(D, B), "bytes": one_byte(D, B)}
    if pieces:
        out["expanding"] = expanding(D, B, pieces)
    out["empty"] = []
    out["half"] = even(D // 2, B // 2, seed=2)
    return out


def pack(docs):
    """(text uint8[total], doc_off int64[n + 1])"""
    off = np.zeros(len(docs) + 1, dtype=np.int64)
    if docs:
        np.cumsum([len(d) for d in docs], out=off[1:])
    return np.frombuffer(b"".join(docs), dtype=np.uint8).copy(), off


def seq_shapes(D, long_len=3000):
    """name -> lengths of the id sequences (or keys) of a batch, for the calls whose bound is the number of sequences alone"""
    mix = [0, 1, 2, 5, 13, 20, 64, 65, 7, 0, 3]
    return {"even": [mix[i % len(mix)] for i in range(D)], "one_long": [long_len if i == D // 2 else 0 for i in range(D)],
            "ones": [1] * D, "empty": [], "half": [mix[(i + 3) % len(mix)] for i in range(D // 2)]}


STREAM_ROW_LENS = (16, 2)                   # of the stream stage: the row length of the other row stages, and one at which `one_long` gives far more rows than sequences


def stream_row_count(lens, L, specials=2):
    """the rows IdsToStreamRowsBatch cuts sequences of these lengths into, every sequence with `specials` ids around it (the last row may be incomplete)"""
    return -(-(sum(lens) + specials * len(lens)) // L)


def hyphenation_words():
    """name -> words of the hyphenation case: the text shapes of the small bound, a document standing for a word (D words, B bytes)"""
    return shapes(*SMALL)


def hyphenation_expected():
    """name -> the reference's WordHyphenationWithModel text per word (tests/golden/ref_answers/word_hyphenation_reserve_contract.json.gz; where
    oracle/_ref is built the live reference is asked and must equal the stored copy)"""
    import w2h_cases as wc
    by_shape = hyphenation_words()
    words = [w for docs in by_shape.values() for w in docs]
    flat = wc.ref_texts("reserve_contract", wc.FIXTURE, words)[str(0x2D)]
    assert len(flat) == len(words), "the stored answers are not those of these words: rewrite them (BF_WRITE_REF_ANSWERS=1)"
    out, k = {}, 0
    for name, docs in by_shape.items():
        out[name] = flat[k:k + len(docs)]
        k += len(docs)
    return out
