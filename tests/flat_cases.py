"""Shared TEST inputs for the flat WordPiece program (blingfire_amd/csrc/bf_flat.h) OFF the corpus it was tuned on: deterministic builders
over the committed data (tests/data/config1_lines.txt.gz, pieces_xlmr.tsv.gz, words_en.txt), used at small size by the simulator tier
(tests/test_flat_emu.py) and at device size by the GPU tier (tests/test_gpu_flat_other_text.py) -- one builder, so both tiers see the same
kind of bytes.  Every builder returns (text uint8, doc_off int64[ndocs + 1]).

The metric's generator (bfutil "headline512" / "config2") gives ASCII words without '[' and without a run of more than 14 letters: no document of
it leaves the flat program.  Here about 1 % (real lines) to about half (multilingual text) of the documents do, so
k_wp_hardlist, the wave program's LIST instance, k_wp_count and k_wp_merge work on a mix of streamed, handed-back, invalid and empty documents."""
import random

import numpy as np

import bfutil

WF_CHUNK = 512                # bf_flat_key.h: bytes of a step of k_wp_flat
WF_RUN_MAX = 48               # bytes of the longest run the flat program resolves itself
WF_DOC_MAX = 1 << 22          # a batch with a longer document is not taken by the flat program

EDGE_LENGTHS = (1, 7, 8, 9, 63, 64, 65, 511, 512, 513, 1023, 1024, 1025, 1536)
EDGE_FILLS = (b"a ", b"ab, ", "é ".encode(), b"word ")
# more words the table does not answer than a range's record list holds: characters the vocabulary lacks, with and without blanks between them
OVERFLOW_BODIES = tuple(s.encode() for s in ("͸ " * 2000, "͸" * 3000, "\U00020000" * 1500, "͸a͹b " * 1200))
# a character the vocabulary does not hold as the very last bytes of the batch (its word is read from the text, character by character)
TAILS = tuple(s.encode() for s in ("tail \U00020000", "tail ๛", "x一"))
SHAPES_ROTATIONS = len(TAILS)


def pack(docs):
    off = np.zeros(len(docs) + 1, dtype=np.int64)
    if docs:
        np.cumsum([len(d) for d in docs], out=off[1:])
    return np.frombuffer(b"".join(docs), dtype=np.uint8).copy(), off


def docs_of(batch):
    text, off = batch
    raw = text.tobytes()
    return [raw[off[d]:off[d + 1]] for d in range(len(off) - 1)]


def headline(n):
    return docs_of(bfutil.gen_workload("headline512", n))


def real_lines(n=30000):
    """the reference's own test lines (42.8 bytes per line, 65 of 10,000 with '[', 22 with a run of more than 48 bytes, 900 outside ASCII, one of
    8,396 bytes); 30,000 lines are 1,283,205 bytes: a fresh handle chooses the flat program by itself"""
    return bfutil.config1_lines(n)


def multilingual(n=4000):
    """config 4's multilingual generator: about half of the documents leave the flat program (runs of more than 48 bytes, record lists that
    overflow); 4,000 documents are 2,051,998 bytes"""
    return bfutil.gen_workload("config4", n)


def mixture(nhead=2400):
    """headline documents with a multilingual document behind every third and an empty one behind every fiftieth: 203 documents per 150 headline
    ones, no multiple of 64, so handed-back, invalid and empty documents share k_wp_merge's blocks of 64 with streamed ones at every alignment"""
    head, multi = headline(nhead), docs_of(multilingual(nhead // 3))
    docs = []
    for i, d in enumerate(head):
        docs.append(d)
        if i % 3 == 2:
            docs.append(multi[i // 3])
        if i % 50 == 49:
            docs.append(b"")
    return pack(docs)


def edge_docs():
    return [(fill * (n // len(fill) + 1))[:n] for n in EDGE_LENGTHS for fill in EDGE_FILLS]


def many_docs(n=24, seed=5):
    """words of 6 .. 14 letters no vocabulary holds, one after the other: more ids per trip of the merge than its buffer holds; up to 400 per document"""
    rnd = random.Random(seed)
    counts = [400, 1, 399] + [rnd.randint(1, 400) for _ in range(n - 3)]
    return [b" ".join(bytes(rnd.choice(b"qzxjkvw") for _ in range(rnd.randint(6, 14))) for _ in range(k)) for k in counts]


def _run_at(run, end):
    """a document of plain words with a run of `run` letters whose last byte is byte end - 1, then plain words up to the next multiple of WF_CHUNK"""
    head = (b"some words and " * 80)[:end - run - 1] + b" "
    body = head + b"r" * run + b" "
    assert len(body) == end + 1
    return body + (b"then more of them " * 40)[:-len(body) % WF_CHUNK]


def run_docs():
    """runs of exactly 48 bytes (the longest the flat program keeps) and 49 bytes (the shortest it hands back) that end exactly at a chunk boundary
    and one byte behind it.  Every document is a multiple of WF_CHUNK long: as the first documents of a batch each starts at a chunk boundary
    of the first range"""
    docs = [_run_at(run, end) for run in (WF_RUN_MAX, WF_RUN_MAX + 1) for end in (WF_CHUNK, WF_CHUNK + 1, 2 * WF_CHUNK, 2 * WF_CHUNK + 1)]
    assert all(len(d) % WF_CHUNK == 0 for d in docs)
    return docs


def overflow_batch(nsurround=100):
    """the record-list overflow bodies alone among headline documents (nothing else in the batch is handed back)"""
    head = headline(nsurround)
    docs, step = [], max(nsurround // (len(OVERFLOW_BODIES) + 1), 1)
    for i, d in enumerate(head):
        docs.append(d)
        if i % step == step - 1 and i // step < len(OVERFLOW_BODIES):
            docs.append(OVERFLOW_BODIES[i // step])
    return pack(docs)


def shapes(rotation=0, nsurround=2000):
    """the GPU counterpart of test_flat_emu.py::test_document_shapes: every item at the start, in the middle and at the end of a batch of `nsurround`
    headline documents, so that many ranges and waves are live.  The batch starts with run_docs() (chunk-aligned there); the item list is rotated by
    `rotation` items per placement, so that the very first, the middle and the very last position see different items; TAILS[rotation] is the last
    document: its character is the last bytes of the batch.  rotation in range(SHAPES_ROTATIONS)"""
    items = edge_docs() + list(OVERFLOW_BODIES) + many_docs()
    head = headline(nsurround)
    tails = [TAILS[(rotation + 1 + k) % len(TAILS)] for k in range(len(TAILS))]          # ends with TAILS[rotation]

    def group(k):
        r = (7 * rotation + 31 * k) % len(items)
        return items[r:] + items[:r]

    docs = run_docs() + group(0) + tails + head[:nsurround // 2] + run_docs() + group(1) + tails + head[nsurround // 2:] + run_docs() + group(2) + tails
    assert docs[-1] == TAILS[rotation]
    return pack(docs)


def size_limits(nsurround=400):
    """documents at the size limit of the flat program among headline documents: one of exactly WF_DOC_MAX bytes whose last token ends on its last
    byte (4 MiB is not "more than WF_DOC_MAX": the batch stays in the flat program; its spans use all 22 position bits), one of 2 MiB + 777 and one
    of 1.5 MiB + 1 bytes.  Ranges whose byte target falls inside a big document are empty.  With bert_base_tok.bin no document is handed back
    (the words k_wp_units has to walk are few enough for the record lists: tests/test_flat_emu.py pins that)"""
    head = headline(nsurround)
    big = (b"word " * 900000)[:WF_DOC_MAX - 4] + b" cat"
    mid = (b"ab, cd. " * 300000)[:(2 << 20) + 777]
    low = ("the café is open , and naïve words follow it here ".encode() * 32000)[:(3 << 19) + 1]      # (two words per 52 bytes for k_wp_units: its list holds them)
    assert len(big) == WF_DOC_MAX
    a, b, c = nsurround // 3, 2 * nsurround // 3, nsurround - 5
    return pack(head[:a] + [big] + head[a:b] + [mid] + head[b:c] + [low] + head[c:])
