// bf_mhclust.h -- MinHash clusters: from LSH band keys (and, optionally, signatures) to the connected components of the candidate graph.
//
// Additive (the reference has no counterpart; include/blingfiretokdll_amd.h MinHashClustersBatchDevice is the specification; it is restated here).
// Integer only, so bit-exact by specification.
//   Inputs.     key = int64 [nseq, B] band keys, sig = int32 [nseq, H] signatures, nshingles = int32 [nseq] or none.  1 <= B <= 256, 1 <= H <= 256.
//   live(q)     no nshingles, or nshingles[q] > 0 (the signature of an empty sequence is all ones: without this rule every empty document would
//               fall into one cluster).
//   f(q, b)     for a live q: the smallest live q' with key[q'][b] == key[q][b].  Keys are compared column by column only; every 64-bit value is
//               a key.  (q, b) is a CANDIDATE when f(q, b) != q.
//   Edges.      A candidate is an edge q -- f when min_equal == 0, or when at least min_equal of the i < H have sig[q][i] == sig[f][i]
//               (MinHashPairsBatchDevice's count).  A member is checked against its band bucket's SMALLEST member, not against every member:
//               with min_equal == 0 the components equal those of all pairs; with min_equal > 0 this is the specification.
//   Outputs.    Clusters = the connected components over 0 .. nseq - 1 (a sequence that is not live is its own).  label[q] = the smallest index
//               of q's component; keep[q] = (label[q] == q); size[q] = the members of q's component; counts = {clusters, candidates}.
//
// The split (bf_kernels_mhclust.hip).  One open-addressing TABLE per band, reused band after band: T = 2 * nseq + 64 slots as two arrays,
// uint64 key[T] and int32 rep[T].  The last slot is the SIDE SLOT of the one key that equals the empty mark (MHC_EMPTY); the R = T - 1 slots in
// front of it are found by range reduction -- the high word of fmix64(key) * R, so R needs no rounding to a power of two -- and probed linearly.
// A slot is claimed by a 64-bit compare-and-swap on key[] from the empty mark; rep[] takes the minimum of the sequences that arrive.  Minimum is
// associative and commutative: f(q, b) does not depend on the order of arrival, although the slot a key ends up in does.  At most nseq keys meet
// R >= 2 * nseq slots, so an empty slot ends every probe sequence long before its bound of R steps.  Nothing locks, nothing spins on another lane.
//
// UNION-FIND lives in label[] itself: parent[q] = q at the start, find() halves the path, unite() hooks the larger root under the smaller with a
// compare-and-swap and goes on from the roots it then finds when the swap fails.  parent[x] <= x holds at every moment, so find() terminates,
// the structure is a forest at every moment, and the root of a finished component is its smallest index whatever the interleaving was.
//
// Everything is written once here as BF_HD code over a memory policy M (the atomics of the device, or plain sequential C++): the kernels run it
// per lane, and a host program can compile the same header.  Plain C++, no HIP types.
#pragma once
#include <stdint.h>
#include "bf_minhash.h"

namespace bfa {

constexpr int MHC_MAX_BANDS = 256;
constexpr uint64_t MHC_EMPTY = 0x4D4843454D505459ull;         // the empty mark of key[] ("MHCEMPTY"; tests/mhclust_cases.py mirrors it)
constexpr int32_t MHC_NONE = 0x7fffffff;                      // rep[] of a slot nobody arrived at
constexpr int64_t MHC_TABLE_EXTRA = 64;

// false = the parameters are refused (BF_E_ARG)
BF_HD bool mhclust_spec(int num_perm, int bands, int64_t nseq, int min_equal, int flags)
{
    return num_perm >= 1 && num_perm <= MINHASH_MAX_PERM && bands >= 1 && bands <= MHC_MAX_BANDS && min_equal >= 0 && min_equal <= num_perm && flags == 0 &&
           nseq >= 0 && nseq < 0x7fffffff;
}

BF_HD int64_t mhclust_slots(int64_t nseq) { return 2 * nseq + MHC_TABLE_EXTRA; }                 // T, the side slot included
BF_HD bool mhclust_live(const int32_t *nshingles, int64_t q) { return !nshingles || nshingles[q] > 0; }

// the high 64 bits of a * b, in 32-bit pieces (no 128-bit type: the same code for both compilers)
BF_HD uint64_t mhclust_mulhi(uint64_t a, uint64_t b)
{
    const uint64_t a0 = (uint32_t)a, a1 = a >> 32, b0 = (uint32_t)b, b1 = b >> 32;
    const uint64_t lo = a0 * b0, m1 = a1 * b0 + (lo >> 32), m2 = a0 * b1 + (uint32_t)m1;
    return a1 * b1 + (m1 >> 32) + (m2 >> 32);
}
// the home slot of a key among R regular slots
BF_HD int64_t mhclust_home(uint64_t key, int64_t R) { return (int64_t)mhclust_mulhi(minhash_fmix64(key), (uint64_t)R); }

// k_mhc_insert, one lane: sequence q arrives with `key`.  T = mhclust_slots(nseq).
template <class M> BF_HD void mhclust_insert(uint64_t *tkey, int32_t *trep, int64_t T, uint64_t key, int32_t q)
{
    const int64_t R = T - 1;
    if (key == MHC_EMPTY) { M::min32(&trep[R], q); return; }
    int64_t s = mhclust_home(key, R);
    for (int64_t probe = 0; probe < R; ++probe) {
        const uint64_t old = M::cas64(&tkey[s], MHC_EMPTY, key);
        if (old == MHC_EMPTY || old == key) { M::min32(&trep[s], q); return; }
        s = s + 1 == R ? 0 : s + 1;
    }
}

// k_mhc_link, one lane: f of a key that was inserted (behind the insert kernel: plain loads).  MHC_NONE for a key that was not.
BF_HD int32_t mhclust_lookup(const uint64_t *tkey, const int32_t *trep, int64_t T, uint64_t key)
{
    const int64_t R = T - 1;
    if (key == MHC_EMPTY) return trep[R];
    int64_t s = mhclust_home(key, R);
    for (int64_t probe = 0; probe < R; ++probe) {
        const uint64_t k = tkey[s];
        if (k == key) return trep[s];
        if (k == MHC_EMPTY) return MHC_NONE;
        s = s + 1 == R ? 0 : s + 1;
    }
    return MHC_NONE;
}

// the root of x, halving the path on the way: parent[x] moves to a grandparent, which is smaller and in x's tree -- whoever else writes
// parent[x] in between (x is no root, so only another find does) writes such a node too
template <class M> BF_HD int32_t mhclust_find(int32_t *parent, int32_t x)
{
    for (;;) {
        const int32_t p = M::load32(&parent[x]);
        if (p == x) return x;
        const int32_t g = M::load32(&parent[p]);
        if (g == p) return p;
        M::cas32(&parent[x], p, g);
        x = g;
    }
}

// joins the components of a and b: the larger root goes under the smaller.  A swap that fails means another lane hooked that root first:
// that lane made progress, and this one goes on from the roots it finds now.
template <class M> BF_HD void mhclust_unite(int32_t *parent, int32_t a, int32_t b)
{
    for (;;) {
        a = mhclust_find<M>(parent, a); b = mhclust_find<M>(parent, b);
        if (a == b) return;
        const int32_t lo = a < b ? a : b, hi = a < b ? b : a;
        if (M::cas32(&parent[hi], hi, lo) == hi) return;
        a = lo; b = hi;
    }
}

// the memory policy of a sequential host program
struct MhcSeq {
    static inline uint64_t cas64(uint64_t *p, uint64_t expect, uint64_t v) { const uint64_t old = *p; if (old == expect) *p = v; return old; }
    static inline int32_t cas32(int32_t *p, int32_t expect, int32_t v) { const int32_t old = *p; if (old == expect) *p = v; return old; }
    static inline void min32(int32_t *p, int32_t v) { if (v < *p) *p = v; }
    static inline int32_t load32(const int32_t *p) { return *p; }
};

} // namespace bfa
