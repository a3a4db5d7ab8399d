"""MinHash over shingles of token ids (IdsToMinHashBatchDevice): the specification restated sequentially, and the case table of the GPU tier.
All arithmetic is unsigned and wraps; an id enters as uint32.  Sequence q = ids[off[q] .. off[q+1]) of n ids has n - k + 1 shingles when n >= k,
one over all its ids when 0 < n < k, none when n = 0.  Shingle hash: s = uint32(seed); per id s = fmix32((s ^ id) + 0x9E3779B9).  Permutation i:
w = philox4x32_10(i, 0, 0, 0x4D48, seed_lo, seed_hi); a = (w1 << 32 | w0) | 1; b = w3 << 32 | w2; h_i(s) = ((a * s + b) mod 2^64) >> 32.
sig[q][i] = min over the shingles, 0xFFFFFFFF with none.  Band b of r words: x = seed ^ ((b + 1) * 0x9E3779B97F4A7C15); per word x = fmix64(x ^ v).
The loops over shingles and permutations are plain Python; only the minimum over a sequence's shingle hashes is numpy's over uint64, whose
products wrap as the specification says (test_minhash_host holds it to Python ints)."""
import numpy as np

from mlm_cases import philox

M32, M64, EMPTY = 0xFFFFFFFF, 0xFFFFFFFFFFFFFFFF, 0xFFFFFFFF
TILE = 1024                       # MINHASH_TILE of bf_minhash.h
KS, HS = (1, 2, 5, 8), (1, 64, 65, 128, 200, 256)


def fmix32(h):
    h = ((h ^ (h >> 16)) * 0x85EBCA6B) & M32
    h = ((h ^ (h >> 13)) * 0xC2B2AE35) & M32
    return h ^ (h >> 16)


def fmix64(x):
    x = ((x ^ (x >> 33)) * 0xFF51AFD7ED558CCD) & M64
    x = ((x ^ (x >> 33)) * 0xC4CEB9FE1A85EC53) & M64
    return x ^ (x >> 33)


def shingle_hash(shingle, seed):
    s = seed & M32
    for t in shingle:
        s = fmix32(((s ^ (int(t) & M32)) + 0x9E3779B9) & M32)
    return s


def perm(seed, i):
    w = [int(x) for x in philox(i, 0, 0, 0x4D48, seed & M32, (seed >> 32) & M32)]
    return ((w[1] << 32) | w[0]) | 1, (w[3] << 32) | w[2]


def shingles(t, k):
    return [] if not t else [t] if len(t) < k else [t[p:p + k] for p in range(len(t) - k + 1)]


def restate(ids, off, k, H, r=0, seed=0):
    """-> dict(sig int32[nseq, H], keys int64[nseq, H / r] or None, nshingles int32[nseq], status)"""
    nseq, status = len(off) - 1, 0
    ab = [tuple(np.uint64(x) for x in perm(seed, i)) for i in range(H)]
    sig, nsh = np.full((nseq, H), EMPTY, dtype=np.uint32), np.zeros(nseq, dtype=np.int32)
    keys = np.zeros((nseq, H // r), dtype=np.uint64) if r else None
    for q in range(nseq):
        b, e = int(off[q]), int(off[q + 1])
        if b < 0 or e < b or e > len(ids):
            status |= 8                                         # read as empty
        else:
            sh = shingles(ids[b:e].tolist(), k)
            nsh[q] = len(sh)
            S = np.array([shingle_hash(s, seed) for s in sh], dtype=np.uint64)
            for i, (a, c) in enumerate(ab if sh else ()):
                sig[q, i] = ((a * S + c) >> np.uint64(32)).min()
        for band in range(H // r if r else 0):
            x = (seed ^ ((band + 1) * 0x9E3779B97F4A7C15)) & M64
            for v in sig[q, band * r:band * r + r].tolist():
                x = fmix64(x ^ v)
            keys[q, band] = x
    return dict(sig=sig.view(np.int32), keys=None if keys is None else keys.view(np.int64), nshingles=nsh, status=status)


def lengths(k):
    """every length the kernel treats differently, laid out so that a sequence ends exactly on a tile edge, a run of empty ones (longer than the
    wave's window of 64 sequences) sits on that edge, a sequence starts on an edge, and one straddles an edge with k - 1 ids on either side"""
    L = [0, 0, 0, 1, k - 1, k, k + 1, 63, 64, 65]
    L.append(TILE - sum(L) % TILE)
    L.extend([0] * 70 + [TILE, TILE - 1, TILE + 1])
    L.append(TILE - max(k - 1, 1) - sum(L) % TILE)
    return L + [2 * max(k - 1, 1), TILE + k - 1, 3 * TILE + 7, 5, 0, 0]


def ragged(lens, seed, base=0):
    """random int32 ids (negative ones, INT32_MIN) for the lengths, `base` unused ids in front: id_offsets[0] = base"""
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64) + base
    ids = np.random.default_rng(seed).integers(-(1 << 31), 1 << 31, size=int(off[-1]), dtype=np.int64).astype(np.int32)
    ids[base:base + 2] = (-(1 << 31), -1)
    return ids, off


def table():
    """(k, H, band_rows, seed, base): k crossed with H, the rest rotating"""
    rot = [((0, 1, 4, H)[i % 4], (0, 1, M64, 0x0123456789ABCDEF)[(i // 2) % 4], (0, 3)[i % 2]) for i, H in enumerate(HS * 4)]
    return [(k, H, r if r and H % r == 0 else 0, s, b) for (k, H), (r, s, b) in zip(((k, H) for k in KS for H in HS), rot)]


def big():
    """one sequence of 200,000 ids among 5,000 of 1 .. 40: the atomic path"""
    lens = np.random.default_rng(7).integers(1, 41, size=5000).tolist()
    return ragged(lens[:2500] + [200000] + lens[2500:], 11)
