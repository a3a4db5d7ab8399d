"""N-gram sets and overlap (IdsToNgramSetBatchDevice, IdsNgramOverlapBatchDevice): the header's specification restated sequentially, and the one
case table of the GPU and the host tier.  All arithmetic is uint64 and wraps; an id enters as uint32.  A sequence of len ids has
max(0, len - n + 1) n-grams.  m(id) = fmix64(seed ^ ((id + 1) * 0x9E3779B97F4A7C15)); P = P * 0x100000001B3 + m(id) over the n-gram;
g = fmix64(P ^ (n * 0xC2B2AE3D27D4EB4F)), 0 read as 1.  The set is a Python set of fingerprints; hits and coverage are loops over starts."""
import functools

import numpy as np

from minhash_cases import M64, fmix64

TILE, LANE, NS = 1024, 16, (1, 2, 13, 16, 17, 64)          # NGRAM_TILE, NGRAM_LANE of bf_ngram.h


def fingerprint(gram, n, seed):
    P = 0
    for t in gram:
        P = (P * 0x100000001B3 + fmix64(seed ^ ((((int(t) & 0xFFFFFFFF) + 1) * 0x9E3779B97F4A7C15) & M64))) & M64
    return fmix64(P ^ ((n * 0xC2B2AE3D27D4EB4F) & M64)) or 1


def prints(ids, off, n, seed):
    """per sequence: (first id cell, length, the fingerprints of its n-grams), a bad range read as empty; and the status word"""
    out, status = [], 0
    for b, e in zip(off[:-1].tolist(), off[1:].tolist()):
        bad = b < 0 or e < b or e > len(ids)
        status |= 8 if bad else 0
        t = [] if bad else ids[b:e].tolist()
        out.append((b, len(t), [fingerprint(t[p:p + n], n, seed) for p in range(len(t) - n + 1)]))
    return out, status


def build(ids, off, n, seed, members=None):
    """-> (the set, counts {read, newly stored, 0}) of a set call that adds to `members`"""
    g = [x for _, _, gs in prints(ids, off, n, seed)[0] for x in gs]
    new = set(g) - (members or set())
    return (members or set()) | new, np.array([len(g), len(new), 0], dtype=np.int64)


def overlap(ids, off, n, seed, members):
    """-> dict(ngrams, hits, covered int32[nseq], mask uint8[len(ids)] with 7 where no sequence holds the cell, status)"""
    seqs, status = prints(ids, off, n, seed)
    out = dict(ngrams=np.array([len(gs) for _, _, gs in seqs], dtype=np.int32), hits=np.zeros(len(seqs), np.int32), covered=np.zeros(len(seqs), np.int32),
               mask=np.full(len(ids), 7, np.uint8), status=status)
    for q, (b, ln, gs) in enumerate(seqs):
        cov = np.zeros(ln, np.uint8)
        for p, g in enumerate(gs):
            if g in members:
                out["hits"][q] += 1
                cov[p:p + n] = 1
        out["covered"][q], out["mask"][b:b + ln] = cov.sum(), cov
    return out


@functools.lru_cache(maxsize=None)
def case(n):
    """-> (probe ids, probe off, set ids, set off).  The probe batch: sequences of 0, n - 1, n and n + 1 ids; one of 2,500 ids that spans two tile
    edges; 3,000 of one and two ids (many inside one lane's 16 positions); one that straddles an edge; a last range that leaves the array.  The
    set batch: n-grams copied from the probe STREAM at chosen starts, relative to the tile edges -- in the last n - 1 positions of a tile (right
    halo of that tile, left halo and bitmap window of the next), ending exactly on an edge, at a lane's positions 0, 15 and 16, and across the
    ends of sequences (no n-gram there: no hit) -- and 30 random ids.  Ids are drawn from 4 to 50 values, INT32_MIN and -1 among them."""
    rng = np.random.default_rng(100 + n)
    vocab = rng.integers(-(1 << 31), 1 << 31, size={1: 50, 2: 12}.get(n, 4), dtype=np.int64).astype(np.int32)
    vocab[:2] = (-(1 << 31), -1)
    lens = [0, n - 1, n, n + 1, 2500, 0, 0] + [1, 2] * 1500 + [0, 2 * TILE + n, 70]
    ids = vocab[rng.integers(0, len(vocab), size=sum(lens))]
    off = np.concatenate([[0], np.cumsum(lens), [sum(lens) + 5]]).astype(np.int64)
    e1, e2, e8 = TILE, 2 * TILE, 8 * TILE
    starts = [n - 1, 2 * n - 1, 3 * n - 1, e1 - (n - 1), e1 - 1, e1 - n, e1 + LANE, e1 + 2 * LANE - 1, e1 + 2 * LANE, e2 - n, e2 - n // 2, 3 * n + 2500 - n,
              3 * n + 2500 - n + 1, e8 - (n - 1), e8 - n // 2, len(ids) - n]
    grams = [ids[s:s + n] for s in starts] + [vocab[rng.integers(0, len(vocab), size=30)]]
    return ids, off, np.concatenate(grams), np.concatenate([[0], np.cumsum([len(g) for g in grams])]).astype(np.int64)
