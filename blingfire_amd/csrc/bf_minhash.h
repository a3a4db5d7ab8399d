// bf_minhash.h -- MinHash signatures and LSH band keys from ragged token ids (near-duplicate detection over shingles of ids).
//
// Additive (the reference has no counterpart; include/blingfiretokdll_amd.h IdsToMinHashBatchDevice is the specification; it is restated here).
// All arithmetic is unsigned and wraps; an id enters as (uint32)id.
//   Shingles.   Sequence q has ids t[0 .. n), n = off[q+1] - off[q].  n >= k: n - k + 1 shingles, one at every start p over t[p .. p + k);
//               0 < n < k: one shingle over all n ids; n = 0: none.  1 <= k <= 8.
//   Hash.       s = (uint32)seed; for each id of the shingle in order s = fmix32((s ^ id) + 0x9E3779B9), fmix32 = the MurmurHash3 finalizer.
//   Permutation i (0 <= i < H, 1 <= H <= 256).  w = philox4x32_10(i, 0, 0, 0x4D48, seed_lo, seed_hi) (bf_mlm.h); a_i = (w[1] << 32 | w[0]) | 1,
//               b_i = w[3] << 32 | w[2]; h_i(s) = (uint32)((a_i * (uint64)s + b_i) >> 32): multiply-shift universal hashing (Dietzfelbinger).
//   Signature.  sig[q][i] = the minimum of h_i(s) over the shingles of q; 0xFFFFFFFF with none.  int32 bit patterns, [nseq, H].
//   Band keys.  band_rows = r > 0 divides H, B = H / r; key[q][b] starts at x = seed ^ ((uint64)(b + 1) * 0x9E3779B97F4A7C15), then for each of
//               the band's r words v in order x = fmix64(x ^ v), fmix64 = the MurmurHash3 64-bit finalizer.  int64, [nseq, B].
//
// The split (bf_kernels_minhash.hip).  The ids of all sequences, laid end to end, are a stream of T positions; W = the exclusive scan of the
// lengths says where a sequence lies in it.  The stream is cut into tiles of MINHASH_TILE positions and a wave takes a tile: a shingle belongs to
// the tile that holds its first id (its other ids are read across the tile's edge).  Inside the wave a LANE OWNS PERMUTATIONS -- lane l keeps a, b
// and the running minimum of the permutations l, l + 64, ... in registers -- and the WAVE WALKS SHINGLES: the hashes of 64 shingles are computed
// one per lane, then each is broadcast in turn and every lane takes one multiply-add and one min per permutation it owns.  Nothing is reduced
// across lanes, and no lane idles because a sequence is short.  At a sequence's end the minima are flushed: a plain store when the sequence lies
// inside one tile (minhash_inside), else an atomic min into a row that was set to all ones before (min is associative and commutative: the bytes
// do not depend on the order).  Everything those decisions depend on is written once here as BF_HD code: the kernels run it per lane, and
// a host program can compile the same header.  Plain C++, no HIP types.
#pragma once
#include <stdint.h>
#include "bf_mlm.h"
#include "bf_stream.h"

namespace bfa {

constexpr int MINHASH_MAX_SHINGLE = 8;
constexpr int MINHASH_MAX_PERM = 256;
constexpr int MINHASH_TILE = 1024;            // stream positions a wave takes at a time (tests/minhash_cases.py mirrors it)
constexpr int MINHASH_CHUNK = 64;             // shingles hashed at once: one per lane
constexpr int MINHASH_MAX_SLOTS = MINHASH_MAX_PERM / 64;      // permutations a lane owns at most
constexpr uint32_t MINHASH_EMPTY = 0xFFFFFFFFu;
constexpr uint32_t MINHASH_PHILOX_TAG = 0x4D48u;              // counter word 3 of the parameter draw ("MH")
constexpr int MINHASH_STATUS_CAP = 1;         // BfLastStatus bit 0: rows beyond sig_cap were not written
constexpr int MINHASH_PARAM_BYTES = MINHASH_MAX_PERM * 16;    // the workspace of the parameters: {a lo, a hi, b lo, b hi} per permutation

struct MinhashSpec {
    int k, H, r, B;                           // shingle, num_perm, band_rows (0 = no keys), bands
    uint64_t seed;
};

// fills `s`; false = the parameters are refused (BF_E_ARG)
BF_HD bool minhash_spec(int shingle, int num_perm, int band_rows, uint64_t seed, int flags, MinhashSpec *s)
{
    if (shingle < 1 || shingle > MINHASH_MAX_SHINGLE || num_perm < 1 || num_perm > MINHASH_MAX_PERM || flags != 0) return false;
    if (band_rows < 0 || (band_rows > 0 && num_perm % band_rows != 0)) return false;
    s->k = shingle; s->H = num_perm; s->r = band_rows; s->B = band_rows > 0 ? num_perm / band_rows : 0; s->seed = seed;
    return true;
}

BF_HD uint32_t minhash_fmix32(uint32_t h)
{
    h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;
    return h;
}
BF_HD uint64_t minhash_fmix64(uint64_t x)
{
    x ^= x >> 33; x *= 0xFF51AFD7ED558CCDull; x ^= x >> 33; x *= 0xC4CEB9FE1A85EC53ull; x ^= x >> 33;
    return x;
}

// the shingle hash, one id at a time: s starts at minhash_seed32(seed)
BF_HD uint32_t minhash_seed32(uint64_t seed) { return (uint32_t)seed; }
BF_HD uint32_t minhash_step(uint32_t s, int32_t id) { return minhash_fmix32((s ^ (uint32_t)id) + 0x9E3779B9u); }

// the parameters of permutation i
struct MinhashPerm { uint64_t a, b; };
BF_HD MinhashPerm minhash_perm(uint64_t seed, int i)
{
    const Philox4 w = philox4x32_10((uint32_t)i, 0u, 0u, MINHASH_PHILOX_TAG, (uint32_t)seed, (uint32_t)(seed >> 32));
    return MinhashPerm{(((uint64_t)w.v[1] << 32) | w.v[0]) | 1ull, ((uint64_t)w.v[3] << 32) | w.v[2]};
}
// h_i(s): the high word of a 64 x 32 multiply-add
BF_HD uint32_t minhash_hash(uint64_t a, uint64_t b, uint32_t s) { return (uint32_t)((a * (uint64_t)s + b) >> 32); }

// the key of band b over its r signature words
BF_HD uint64_t minhash_band_key(uint64_t seed, int b, const uint32_t *words, int r)
{
    uint64_t x = seed ^ ((uint64_t)(b + 1) * 0x9E3779B97F4A7C15ull);
    for (int j = 0; j < r; ++j) x = minhash_fmix64(x ^ (uint64_t)words[j]);
    return x;
}

// the length of sequence [b, e) of the ids as the stream counts it: a bad range (rows_seq_len) and a sequence of more than STREAM_MAX_IDS ids
// (the lengths are scanned as int32) are read as empty
BF_HD int32_t minhash_len(int64_t b, int64_t e, int64_t ids_len, bool *bad)
{
    int64_t n = rows_seq_len(b, e, ids_len, bad);
    if (n > STREAM_MAX_IDS) { n = 0; *bad = true; }
    return (int32_t)n;
}
BF_HD int32_t minhash_nshingles(int32_t n, int k) { return n == 0 ? 0 : n < k ? 1 : n - k + 1; }
// ids a shingle of a sequence of n ids holds
BF_HD int minhash_width(int32_t n, int k) { return n < k ? (int)n : k; }

// the tiles: tile j holds the stream positions [j * TILE, (j + 1) * TILE)
BF_HD int64_t minhash_ntiles(int64_t T) { return (T + MINHASH_TILE - 1) / MINHASH_TILE; }
// a non-empty sequence at stream positions [w0, w1) lies inside one tile: its row is flushed once, with a plain store.  Every other row --
// the sequences that span a tile's edge, and the empty ones, which no tile meets -- is set to all ones by k_mh_init (minhash_init_row).
BF_HD bool minhash_inside(int64_t w0, int64_t w1) { return w1 > w0 && w0 / MINHASH_TILE == (w1 - 1) / MINHASH_TILE; }
BF_HD bool minhash_init_row(int64_t w0, int64_t w1) { return !minhash_inside(w0, w1); }

// The shingle starts of a sequence (n ids at stream positions [w0, w0 + n)) that tile [t0, t0 + TILE) owns: x in [*x0, *x1), relative to the
// sequence; empty when *x0 >= *x1.  A start x reads the ids x .. x + minhash_width(n, k) - 1, all inside the sequence.
BF_HD void minhash_starts(int64_t w0, int32_t n, int k, int64_t t0, int32_t *x0, int32_t *x1)
{
    const int64_t lo = t0 > w0 ? t0 - w0 : 0, hi = t0 + MINHASH_TILE - w0;
    const int32_t ns = minhash_nshingles(n, k);
    *x0 = lo < ns ? (int32_t)lo : ns;
    *x1 = hi < ns ? (int32_t)hi : ns;
}

// the pairs kernel: lanes that compare one pair -- a power of two that holds H, a whole wave from 33 on
BF_HD int minhash_pair_slice(int H) { int s = 1; while (s < H && s < 64) s <<= 1; return s; }

} // namespace bfa
