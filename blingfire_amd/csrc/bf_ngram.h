// bf_ngram.h -- exact n-gram overlap of ragged token ids against a set of n-gram fingerprints that outlives a call (benchmark decontamination,
// block lists, filtering a batch against one already seen).
//
// Additive (the reference has no counterpart; include/blingfiretokdll_amd.h IdsToNgramSetBatchDevice / IdsNgramOverlapBatchDevice is the
// specification; it is restated here).  All arithmetic is uint64 and wraps; an id enters as (uint32)id.
//   Sequences.   Read as in IdsToMinHashBatchDevice (minhash_len): a bad range, or more than STREAM_MAX_IDS ids, is read as empty (status bit 3).
//   N-grams.     A sequence of len ids has max(0, len - n + 1) n-grams, one at every start p over t[p .. p + n), 1 <= n <= 64.
//   Fingerprint. m(id) = fmix64(seed ^ (((uint64)(uint32)id + 1) * 0x9E3779B97F4A7C15)); P = 0, for each id in order P = P * B + m(id) with
//                B = 0x100000001B3; g = fmix64(P ^ ((uint64)n * 0xC2B2AE3D27D4EB4F)); a g of 0 is stored and looked up as 1 (0 = empty).
//   Table.       uint64 table[slots], slots >= 2, 0 = empty.  Home = the high 64 bits of g * slots; linear probing that wraps, at most `slots`
//                steps; insert = a 64-bit compare-and-swap from 0, an equal value found = already present.
//   Set call.    counts = {n-grams read, fingerprints newly stored, n-grams that found no slot}; the third > 0 sets status bit 0.
//   Overlap.     ngrams[q]; hits[q] = starts whose fingerprint is in the table; covered[q] = ids inside at least one hit n-gram; mask per id.
//
// The split (bf_kernels_ngram.hip).  The ids of all sequences laid end to end are a stream of T positions, W = the exclusive scan of the lengths
// (MinHash's).  The stream is cut into tiles of NGRAM_TILE positions and a wave takes a tile; a LANE OWNS NGRAM_LANE = 16 CONSECUTIVE POSITIONS.
//   stage    m(id) of the tile and of n - 1 positions on either side goes to LDS as uint64, once per id: a lane stages its own 16 positions,
//            walking the sequences they lie in (ngram_stage_own), and one position of each halo (ngram_stage_at).  Staged position u sits at
//            index u - t0 + NGRAM_HALO, SKEWED by one pad qword per 16 (ngram_lds): lane bases are then 17 qwords = 34 banks apart, so the 32
//            lanes of one pass of a ds_read_b64 fall on 32 different bank pairs instead of on two.
//   prints   the lane evaluates P of its first start by Horner (n steps) and rolls to the next 15: P' = (P - m[p] * B^(n-1)) * B + m[p + n],
//            two LDS reads and two multiplies a position whatever n is (ngram_prints).  The identity holds in wrapping arithmetic for whatever
//            the cells hold, so a start whose n-gram is not valid may roll over cells nobody staged: its fingerprint is never used.
//   probe    the 16 fingerprints stay in registers; the 16 home-slot loads are issued together and only then are collisions followed
//            (ngram_probe16): the gathers are independent and wait for one latency, not sixteen.  The set call inserts instead (ngram_insert).
//   cover    each lane's 16 hit bits go into a bitmap in LDS (bit = start - t0 + 64; the n - 1 starts left of the tile are probed again by this
//            tile and land in word 0).  Position t is covered when a bit of [t - n + 1, t] is set: a 64-bit window at a bit offset (ngram_window).
//   counts   a lane adds up runs of equal sequence over its 16 positions (ngram_runs): a plain store when the sequence lies inside the lane's 16
//            positions (ngram_inside), else a 32-bit atomic add into a row that an init kernel zeroed.  Integer addition is associative and
//            commutative: the bytes do not depend on the order.
// Everything a lane decides is written once here as BF_HD code over a memory policy M (the atomics of the device, or plain sequential C++): the
// kernels run it per lane, and a host program can compile the same header.  Plain C++, no HIP types.
#pragma once
#include <stdint.h>
#include "bf_mhclust.h"

namespace bfa {

constexpr int NGRAM_MAX = 64;
constexpr int NGRAM_TILE = MINHASH_TILE;                 // stream positions a wave takes at a time (tests/ngram_cases.py mirrors it)
constexpr int NGRAM_LANE = 16;                           // consecutive positions a lane owns: 64 x 16 = NGRAM_TILE
constexpr int NGRAM_HALO = NGRAM_MAX - 1;                // positions staged on either side of the tile, at most
constexpr int NGRAM_STAGE = NGRAM_TILE + 2 * NGRAM_HALO; // staged positions, at most
constexpr int NGRAM_STAGE_QWORDS = NGRAM_STAGE + NGRAM_STAGE / 16 + 1;       // with the skew: 9,776 bytes
constexpr int NGRAM_BM_BASE = 64;                        // bit of the start at t0
constexpr int NGRAM_BM_WORDS = (NGRAM_BM_BASE + NGRAM_TILE) / 64 + 1;        // and one word of zeros behind, for the window's second read
constexpr uint64_t NGRAM_B = 0x100000001B3ull;
constexpr int NGRAM_SET_CLEAR = 1;                       // flags bit 0 of the set call
constexpr int NGRAM_STATUS_FULL = 1;                     // BfLastStatus bit 0: an n-gram found no slot
constexpr int64_t NGRAM_SLOTS_EXTRA = 64;                // the wrappers' default table: 2 * ids_len + 64 slots

// false = the parameters both calls share are refused (BF_E_ARG)
BF_HD bool ngram_spec(int n, int64_t slots, int64_t nseq, int64_t ids_len) { return n >= 1 && n <= NGRAM_MAX && slots >= 2 && nseq >= 0 && nseq <= 0x7fffffff && ids_len >= 0; }

BF_HD int32_t ngram_count(int32_t len, int n) { return len >= n ? len - n + 1 : 0; }
BF_HD uint64_t ngram_m(uint64_t seed, int32_t id) { return minhash_fmix64(seed ^ (((uint64_t)(uint32_t)id + 1ull) * 0x9E3779B97F4A7C15ull)); }
BF_HD uint64_t ngram_final(uint64_t P, int n) { const uint64_t g = minhash_fmix64(P ^ ((uint64_t)n * 0xC2B2AE3D27D4EB4Full)); return g ? g : 1ull; }
// B^(n-1), the weight of the id that leaves a rolling window (computed on the host, a kernel argument)
BF_HD uint64_t ngram_pow(int n) { uint64_t x = 1; for (int i = 1; i < n; ++i) x *= NGRAM_B; return x; }
BF_HD uint64_t ngram_roll(uint64_t P, uint64_t m_out, uint64_t m_in, uint64_t bpow) { return (P - m_out * bpow) * NGRAM_B + m_in; }

// the skewed LDS index of staged cell i (i = position - t0 + NGRAM_HALO): one pad qword per 16
BF_HD int ngram_lds(int i) { return i + (i >> 4); }
BF_HD int ngram_lane_cell(int lane) { return NGRAM_HALO + NGRAM_LANE * lane; }       // the staged cell of a lane's first position

BF_HD int64_t ngram_ntiles(int64_t T) { return (T + NGRAM_TILE - 1) / NGRAM_TILE; }
// a non-empty sequence at stream positions [w0, w1) lies inside the 16 positions of one lane (tiles and lanes are aligned to 16): its counts are
// stored once, plainly.  Every other row -- the sequences several lanes add to, and the empty ones, which no lane meets -- is zeroed first.
BF_HD bool ngram_inside(int64_t w0, int64_t w1) { return w1 > w0 && (w0 >> 4) == ((w1 - 1) >> 4); }

// ---- the table
BF_HD int64_t ngram_home(uint64_t g, int64_t slots) { return (int64_t)mhclust_mulhi(g, (uint64_t)slots); }
enum { NGRAM_STORED = 0, NGRAM_PRESENT = 1, NGRAM_NO_SLOT = 2 };
template <class M> BF_HD int ngram_insert(uint64_t *table, int64_t slots, uint64_t g)
{
    int64_t s = ngram_home(g, slots);
    for (int64_t probe = 0; probe < slots; ++probe) {
        const uint64_t old = M::cas64(&table[s], 0ull, g);
        if (old == 0ull) return NGRAM_STORED;
        if (old == g) return NGRAM_PRESENT;
        s = s + 1 == slots ? 0 : s + 1;
    }
    return NGRAM_NO_SLOT;
}
// the look-up from the home slot s, whose value v is already there: at most `slots` slots are looked at
BF_HD bool ngram_chase(const uint64_t *table, int64_t slots, uint64_t g, int64_t s, uint64_t v)
{
    for (int64_t probe = 1; v != g && v != 0ull && probe < slots; ++probe) {
        s = s + 1 == slots ? 0 : s + 1;
        v = table[s];
    }
    return v == g;
}
BF_HD bool ngram_lookup(const uint64_t *table, int64_t slots, uint64_t g)
{
    const int64_t s = ngram_home(g, slots);
    return ngram_chase(table, slots, g, s, table[s]);
}
// the hit bits of a lane's 16 fingerprints (0 = no n-gram there): every home slot is loaded before any collision is followed
BF_HD uint32_t ngram_probe16(const uint64_t *table, int64_t slots, const uint64_t *g)
{
    int64_t s[NGRAM_LANE];
    uint64_t v[NGRAM_LANE];
    BF_STREAM_UNROLL
    for (int k = 0; k < NGRAM_LANE; ++k) s[k] = ngram_home(g[k], slots);
    BF_STREAM_UNROLL
    for (int k = 0; k < NGRAM_LANE; ++k) v[k] = table[s[k]];                  // (g == 0 reads slot 0 and is not looked at)
    uint32_t hits = 0;
    BF_STREAM_UNROLL
    for (int k = 0; k < NGRAM_LANE; ++k)
        if (g[k] != 0ull && ngram_chase(table, slots, g[k], s[k], v[k])) hits |= 1u << k;
    return hits;
}

// ---- a tile as its lanes see it: the positions [t0, t1) of a stream of T, and the sequences [qa, qe] that hold every staged position
// (src = StreamGlobal{W, off, qa, qe, 0}: src.at(t, u) = the sequence of position t, where u is a sequence at or in front of it)
struct NgramTile { int64_t t0, t1, T; int n; uint64_t seed, bpow; };
BF_HD int64_t ngram_stage_lo(int64_t t0, int n) { return t0 > n - 1 ? t0 - (n - 1) : 0; }
BF_HD int64_t ngram_stage_hi(int64_t t1, int64_t T, int n) { return t1 + (n - 1) < T ? t1 + (n - 1) : T; }       // exclusive

// stage: the lane's own positions.  *first = the sequence of its first position (kept for ngram_runs), *vmask = bit k: an n-gram starts at
// position k of the lane (it lies in one sequence).  A lane behind t1 stages nothing and has no bits.
template <class Src>
BF_HD void ngram_stage_own(const NgramTile &tl, const Src &src, const int32_t *ids, int lane, uint64_t *sm, StreamUnit *first, uint32_t *vmask)
{
    const int64_t p0 = tl.t0 + NGRAM_LANE * lane;
    *vmask = 0;
    if (p0 >= tl.t1) return;
    StreamUnit u = src.at(p0, src.first());
    *first = u;
    const int cell = ngram_lane_cell(lane);
    uint32_t vm = 0;
    BF_STREAM_UNROLL
    for (int k = 0; k < NGRAM_LANE; ++k) {
        const int64_t t = p0 + k;
        if (t < tl.t1) {
            u = src.at(t, u);
            sm[ngram_lds(cell + k)] = ngram_m(tl.seed, ids[t + u.delta]);
            if (t + tl.n <= u.w1) vm |= 1u << k;
        }
    }
    *vmask = vm;
}
// stage: one position of a halo into staged cell `cell`; true = an n-gram starts there
template <class Src>
BF_HD bool ngram_stage_at(const NgramTile &tl, const Src &src, const int32_t *ids, int64_t t, int cell, uint64_t *sm)
{
    const StreamUnit u = src.at(t, src.first());
    sm[ngram_lds(cell)] = ngram_m(tl.seed, ids[t + u.delta]);
    return t + tl.n <= u.w1;
}
// the halo positions of lane j < n - 1: -1 = none.  Left: t0 - (n - 1) + j; right: t1 + j, behind a full tile only.
BF_HD int64_t ngram_left_pos(const NgramTile &tl, int j) { const int64_t t = tl.t0 - (tl.n - 1) + j; return j < tl.n - 1 && t >= 0 ? t : -1; }
BF_HD int64_t ngram_right_pos(const NgramTile &tl, int j) { const int64_t t = tl.t1 + j; return j < tl.n - 1 && t < tl.T ? t : -1; }
BF_HD int ngram_pos_cell(const NgramTile &tl, int64_t t) { return (int)(t - tl.t0) + NGRAM_HALO; }

// prints: P of the n-gram that starts in staged cell `cell`, by Horner
BF_HD uint64_t ngram_horner(const uint64_t *sm, int cell, int n)
{
    uint64_t P = 0;
    for (int i = 0; i < n; ++i) P = P * NGRAM_B + sm[ngram_lds(cell + i)];
    return P;
}
// prints: the lane's 16 fingerprints, 0 where vmask has no bit: Horner at the first start, then the roll
BF_HD void ngram_prints(const NgramTile &tl, const uint64_t *sm, int lane, uint32_t vmask, uint64_t *g)
{
    const int cell = ngram_lane_cell(lane);
    uint64_t P = ngram_horner(sm, cell, tl.n);
    BF_STREAM_UNROLL
    for (int k = 0; k < NGRAM_LANE; ++k) {
        g[k] = ((vmask >> k) & 1u) ? ngram_final(P, tl.n) : 0ull;
        if (k + 1 < NGRAM_LANE) P = ngram_roll(P, sm[ngram_lds(cell + k)], sm[ngram_lds(cell + k + tl.n)], tl.bpow);
    }
}

// cover: the bitmap.  A lane's 16 hit bits: four lanes share a word.  A start left of the tile: word 0.
template <class M> BF_HD void ngram_put_hits(uint64_t *bm, int lane, uint32_t hits)
{
    if (hits) M::lds_or64(&bm[NGRAM_BM_BASE / 64 + (lane >> 2)], (uint64_t)hits << (16 * (lane & 3)));
}
template <class M> BF_HD void ngram_put_left(const NgramTile &tl, uint64_t *bm, int64_t t) { M::lds_or64(&bm[0], 1ull << (int)(t - tl.t0 + NGRAM_BM_BASE)); }
// the hit bits of the starts [r - n + 1, r] (r = position - t0): non-zero = the position lies inside a hit n-gram.  No clipping at the
// sequence's start is needed: a hit start s in an EARLIER sequence ends there, s + n - 1 < w0 <= t, so s < t - n + 1 lies in front of the
// window; and a start behind t is not in it either.  Every set bit of the window is a start of t's own sequence whose n-gram holds t.
BF_HD uint64_t ngram_window(const uint64_t *bm, int r, int n)
{
    const int o = r + NGRAM_BM_BASE + 1 - n, w = o >> 6, sh = o & 63;
    const uint64_t x = sh ? (bm[w] >> sh) | (bm[w + 1] << (64 - sh)) : bm[w];
    return n == 64 ? x : x & ((1ull << n) - 1ull);
}

// counts: one run of positions of sequence u is finished
template <class M> BF_HD void ngram_flush(const StreamUnit &u, int32_t h, int32_t c, int32_t *hits, int32_t *covered)
{
    const bool own = ngram_inside(u.w0, u.w1);
    if (hits) { if (own) hits[u.q] = h; else if (h) M::add32(&hits[u.q], h); }
    if (covered) { if (own) covered[u.q] = c; else if (c) M::add32(&covered[u.q], c); }
}
// counts and the mask over the lane's positions: `first` and `hmask` are the lane's from the passes before
template <class M, class Src>
BF_HD void ngram_runs(const NgramTile &tl, const Src &src, const StreamUnit &first, int lane, const uint64_t *bm, uint32_t hmask, int32_t *hits, int32_t *covered,
                      uint8_t *mask)
{
    const int64_t p0 = tl.t0 + NGRAM_LANE * lane;
    if (p0 >= tl.t1) return;
    StreamUnit u = first;
    int32_t h = 0, c = 0;
    BF_STREAM_UNROLL
    for (int k = 0; k < NGRAM_LANE; ++k) {
        const int64_t t = p0 + k;
        if (t < tl.t1) {
            if (t >= u.w1) { ngram_flush<M>(u, h, c, hits, covered); h = 0; c = 0; u = src.at(t, u); }
            const bool cov = ngram_window(bm, (int)(t - tl.t0), tl.n) != 0ull;
            h += (int32_t)((hmask >> k) & 1u); c += cov ? 1 : 0;
            if (mask) mask[t + u.delta] = cov ? 1 : 0;
        }
    }
    ngram_flush<M>(u, h, c, hits, covered);
}

// the memory policy of a sequential host program
struct NgramSeq {
    static inline uint64_t cas64(uint64_t *p, uint64_t expect, uint64_t v) { const uint64_t old = *p; if (old == expect) *p = v; return old; }
    static inline void lds_or64(uint64_t *p, uint64_t v) { *p |= v; }
    static inline void add32(int32_t *p, int32_t v) { *p += v; }
};

} // namespace bfa
