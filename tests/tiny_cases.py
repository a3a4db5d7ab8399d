"""Shared TEST inputs: batches of very many tiny documents (search queries, titles, single words, table cells) -- the shape in which one wave of
the wave programs (blingfire_amd/csrc/bf_wave_body.h, bf_bpe_wave_body.h) opens document after document and carries its table of open documents,
its 8-bit entry numbers and its ring base from one to the next, and in which a 512-byte chunk of the flat program holds hundreds of documents.
Deterministic builders over a table of distinct documents, used at small size by the simulator tier (tests/test_tiny_cases_host.py) and at device size
by the GPU tier (tests/test_gpu_tiny_documents.py).  Every builder returns (text uint8, doc_off int64[ndocs + 1]) and asserts its own invariants; the
*_index forms return the index of every document in table(), so that an answer which depends on the document alone is computed once per distinct one."""
import numpy as np

import bfutil
from flat_cases import WF_DOC_MAX

WORD_MAX = 12                 # bytes of the longest word of tests/data/words_en.txt the table takes
DOC_MAX = 16                  # no document of queries() / ones() is longer
RUN_MIN = 70                  # consecutive empty documents: more than a grab of 8, more than a block of 64 (k_wp_count / k_wp_merge)
RUNS = (97, 71, 131)          # queries(): the runs at the very start, in the middle and at the very end
SPECIALS = ("é".encode(), "好".encode(), "\U0001F600".encode(), b"\xef\xbb\xbf", b"\xef\xbb\xbfa", b"to be", b"[UNK]", b"[", b"##ing", b".", b" ")
ONES_EVERY = 37               # ones(): an empty document follows every 37th one-byte document
ONES_HEAVY = (ord("a"), ord("."), ord(" "))

_table = None


def table():
    """(docs, blob uint8, start int64[ndocs], length int64[ndocs], nothers): document 0 is empty, documents 1 .. nothers are every one-byte document
    0x00 .. 0xFF (lone lead and continuation bytes among them) and SPECIALS, the rest are the words of at most WORD_MAX bytes"""
    global _table
    if _table is None:
        others = [bytes([b]) for b in range(256)] + [s for s in SPECIALS if len(s) != 1]
        words = [w.encode() for w in open(bfutil.WORDS_EN).read().split()]
        words = [w for w in words if len(w) <= WORD_MAX]
        docs = [b""] + others + words
        assert len(set(docs)) == len(docs) and max(len(d) for d in docs) <= DOC_MAX and all(s in docs for s in SPECIALS)
        length = np.array([len(d) for d in docs], dtype=np.int64)
        start = np.concatenate([[0], np.cumsum(length)[:-1]]).astype(np.int64)
        _table = (docs, np.frombuffer(b"".join(docs), dtype=np.uint8).copy(), start, length, len(others))
    return _table


def expand(values, start, length, index):
    """ragged gather: for every i the slice values[start[index[i]] : start[index[i]] + length[index[i]]], concatenated -> (flat, offsets int64[n + 1])"""
    n = length[index]
    off = np.zeros(len(index) + 1, dtype=np.int64)
    np.cumsum(n, out=off[1:])
    src = np.repeat(start[index] - off[:-1], n) + np.arange(int(off[-1]), dtype=np.int64)
    return values[src], off


def pack_index(index):
    _, blob, start, length, _ = table()
    return expand(blob, start, length, index)


def _mix(i, salt):
    """a fixed 32-bit scramble of the document number (no generator whose stream a library may change)"""
    x = (i.astype(np.uint64) + np.uint64(salt)) * np.uint64(0x9E3779B97F4A7C15)
    x ^= x >> np.uint64(29)
    x *= np.uint64(0xBF58476D1CE4E5B9)
    return (x >> np.uint64(32)).astype(np.int64)


def longest_runs(empty):
    """(length of the run of True at the very start, at the very end, the lengths of all runs)"""
    e = np.concatenate([[False], empty, [False]]).astype(np.int8)
    d = np.diff(e)
    a, z = np.flatnonzero(d == 1), np.flatnonzero(d == -1)
    runs = z - a
    first = int(runs[0]) if len(a) and a[0] == 0 else 0
    last = int(runs[-1]) if len(z) and z[-1] == len(empty) else 0
    return first, last, runs


def queries_index(n):
    docs, _, _, length, nothers = table()
    assert n >= 4000, "queries(n): too few documents for its shares and runs"
    i = np.arange(n, dtype=np.int64)
    with np.errstate(over="ignore"):
        r = _mix(i, 1) % 100
    word, other = r < 60, (r >= 60) & (r < 85)
    index = np.zeros(n, dtype=np.int64)
    nwords = len(docs) - 1 - nothers
    index[word] = 1 + nothers + (np.arange(int(word.sum()), dtype=np.int64) * 7919) % nwords          # (7919 is prime to the number of words: every word in turn)
    index[other] = 1 + np.arange(int(other.sum()), dtype=np.int64) % nothers                          # every other distinct document in turn
    mid = n // 2
    index[:RUNS[0]] = 0
    index[mid:mid + RUNS[1]] = 0
    index[n - RUNS[2]:] = 0
    # invariants
    empty = index == 0
    first, last, runs = longest_runs(empty)
    assert first >= RUN_MIN and last >= RUN_MIN and int((runs >= RUN_MIN).sum()) >= 3, (first, last)
    share = empty.sum() / n
    assert 0.13 <= share <= 0.17 + sum(RUNS) / n, share
    live = n - empty.sum()
    slack = sum(RUNS) / n                                    # (the three runs replace documents of every kind)
    assert 0.55 - slack <= (index > nothers).sum() / n <= 0.65 and 0.20 - slack <= ((index > 0) & (index <= nothers)).sum() / n <= 0.30
    assert int(length[index].max()) <= DOC_MAX and live > 0
    assert len(np.unique(index[(index > 0) & (index <= nothers)])) == nothers, "queries(n): not every distinct document is there"
    return index


def queries(n):
    """about 60 % words, 25 % of the other distinct documents, 15 % empty documents, three runs of RUNS empty documents (start, middle, end)"""
    text, off = pack_index(queries_index(n))
    assert len(np.unique(text)) == 256 and int(np.diff(off).max()) <= DOC_MAX
    return text, off


def ones_index(n):
    """n one-byte documents and an empty one behind every ONES_EVERY-th of them: n + n // ONES_EVERY documents"""
    assert n >= 2 * 304
    cycle = []
    for b in range(256):                                   # all 256 values; 'a', '.' and the blank again after every 16 of them
        cycle.append(b)
        if b % 16 == 15:
            cycle += ONES_HEAVY
    cycle = np.array(cycle, dtype=np.int64)
    j = np.arange(n, dtype=np.int64)
    one = 1 + cycle[j % len(cycle)]                        # (table(): document 1 + b is the byte b)
    total = n + n // ONES_EVERY
    index = np.zeros(total, dtype=np.int64)
    at = j + j // ONES_EVERY                               # the place of the j-th one-byte document
    index[at] = one
    # invariants
    empty = index == 0
    assert int(empty.sum()) == n // ONES_EVERY and not empty[0] and bool(empty[ONES_EVERY]) and not (empty[1:] & empty[:-1]).any()
    counts = np.bincount(index[~empty] - 1, minlength=256)
    assert counts.min() >= 1 and len(counts) == 256
    plain = np.delete(counts, ONES_HEAVY).max()
    assert all(counts[b] >= 10 * plain for b in ONES_HEAVY), "ones(n): 'a', '.' and the blank are not over-represented"
    return index


def ones(n):
    text, off = pack_index(ones_index(n))
    lens = np.diff(off)
    assert len(text) == n and int(lens.max()) == 1 and int((lens == 0).sum()) == n // ONES_EVERY and len(np.unique(text)) == 256
    # some 512-byte chunks hold more documents than bytes
    assert (np.searchsorted(off, 512, side="right") - 1) > 512
    return text, off


def empties(n):
    text, off = np.zeros(0, dtype=np.uint8), np.zeros(n + 1, dtype=np.int64)
    assert len(off) - 1 == n and int(off[-1]) == 0
    return text, off


def giant():
    """a document five bytes longer than the flat program takes (tests/test_gpu_parity_wp.py test_flat_program_batch_not_fit builds the same)"""
    g = (b"word " * 900000)[:WF_DOC_MAX + 5]
    assert len(g) == WF_DOC_MAX + 5
    return np.frombuffer(g, dtype=np.uint8)


def with_giant(batch):
    """the batch with one document of WF_DOC_MAX + 5 bytes in its middle: k_wp_pre calls the batch unfit, every document goes to the wave program's
    LIST instance.  Returns (text, doc_off); the giant is document (ndocs of the batch) // 2"""
    text, off = batch
    g = giant()
    mid = (len(off) - 1) // 2
    cut = int(off[mid])
    out = np.concatenate([text[:cut], g, text[cut:]])
    noff = np.concatenate([off[:mid + 1], off[mid:] + len(g)])
    lens = np.diff(noff)
    assert len(noff) == len(off) + 1 and int(lens[mid]) == WF_DOC_MAX + 5 and int(noff[-1]) == len(out)
    assert np.array_equal(np.delete(lens, mid), np.diff(off)) and int(np.delete(lens, mid).max(initial=0)) <= WF_DOC_MAX
    return out, noff
