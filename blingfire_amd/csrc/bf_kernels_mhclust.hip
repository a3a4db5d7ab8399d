// bf_kernels_mhclust.hip -- LSH band keys -> clusters of near-duplicates: a hash table per band, verified links, union-find
// (bf_mhclust.h has the lane code, the specification and the split; include/blingfiretokdll_amd.h MinHashClustersBatchDevice is the contract).
//
//  k_mhc_begin    lane per sequence: label[q] = q (every sequence a root), its member count 0; the two counts of the call 0.
//  per band, the table reused:
//  k_mhc_clear    lane per slot: the empty mark in key[], MHC_NONE in rep[].
//  k_mhc_insert   lane per live sequence: claims the slot of its key (64-bit compare-and-swap from the empty mark, linear probing) and leaves
//                 the minimum of the arrivals in rep[]: the bucket's smallest member, whatever the order.
//  k_mhc_link     lane per live sequence looks up f; a ballot counts the candidates (one atomic add per wave).  With min_equal == 0 every
//                 candidate lane unites q and f.  Otherwise the candidates whose ends do not share a root yet (an edge inside a component
//                 changes nothing, verified or not) are compacted by ballot / mbcnt into the wave's LDS slot, and SLICES of lanes --
//                 minhash_pair_slice(H) lanes per candidate, the partition of k_mh_pairs -- read the two signature rows coalesced, count the
//                 equal words by ballot and popcount, and the slice's first lane unites the pair when the count reaches min_equal.
//  tail:
//  k_mhc_flatten  lane per sequence: label[q] = find(q), keep[q], one atomic add per member into the root's count, the cluster count per wave.
//  k_mhc_sizes    size[q] = the count of label[q]; launched only when size is taken.
// Every store to global memory is a vector store or an atomic.  What is indexed: sequences below nseq, slots below T, f < q, LDS cells below 64.
#include "bf_kernels_common.h"

namespace bfa {

// the memory policy of the device: the atomics execute in the L2, and a word other lanes update there is read past the CU's vector cache
struct MhcDev {
    static __device__ __forceinline__ uint64_t cas64(uint64_t *p, uint64_t expect, uint64_t v)
    {
        return (uint64_t)atomicCAS((unsigned long long *)p, (unsigned long long)expect, (unsigned long long)v);
    }
    static __device__ __forceinline__ int32_t cas32(int32_t *p, int32_t expect, int32_t v) { return atomicCAS(p, expect, v); }
    static __device__ __forceinline__ void min32(int32_t *p, int32_t v) { atomicMin(p, v); }
    static __device__ __forceinline__ int32_t load32(const int32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
};

__global__ __launch_bounds__(256) void k_mhc_begin(MhclustParams p)
{
    const int64_t stride = (int64_t)gridDim.x * 256;
    if (blockIdx.x == 0 && threadIdx.x < 2) p.counts[threadIdx.x] = 0ull;
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < p.nseq; q += stride) { p.label[q] = (int32_t)q; p.sizes[q] = 0; }
}

__global__ __launch_bounds__(256) void k_mhc_clear(MhclustParams p)
{
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < p.T; i += stride) { p.tkey[i] = MHC_EMPTY; p.trep[i] = MHC_NONE; }
}

__global__ __launch_bounds__(256) void k_mhc_insert(MhclustParams p, int band)
{
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < p.nseq; q += stride)
        if (mhclust_live(p.nshingles, q)) mhclust_insert<MhcDev>(p.tkey, p.trep, p.T, (uint64_t)p.keys[q * p.B + band], (int32_t)q);
}

__global__ __launch_bounds__(256) void k_mhc_link(MhclustParams p, int band)
{
    __shared__ int32_t s_q[4][64], s_f[4][64];
    const int lane = lane_id(), wave = wave_in_block(), H = p.H;
    const int S = minhash_pair_slice(H), per = 64 / S, sub = lane / S, l = lane & (S - 1);
    const unsigned long long slice = S == 64 ? ~0ull : ((1ull << S) - 1ull);
    const int64_t nwaves = (int64_t)gridDim.x * 4;
    unsigned long long ncand = 0;                               // the wave's: every lane holds the same number
    for (int64_t base = ((int64_t)blockIdx.x * 4 + wave) * 64; base < p.nseq; base += nwaves * 64) {
        const int64_t q = base + lane;
        int32_t f = MHC_NONE;
        if (q < p.nseq && mhclust_live(p.nshingles, q)) f = mhclust_lookup(p.tkey, p.trep, p.T, (uint64_t)p.keys[q * p.B + band]);
        const bool cand = f < (int32_t)q;                       // (a live q finds f <= q; a lane without a sequence holds MHC_NONE and q > 0)
        ncand += (unsigned long long)__popcll(__ballot(cand));
        if (p.min_equal == 0) {
            if (cand) mhclust_unite<MhcDev>(p.label, (int32_t)q, f);
            continue;
        }
        const bool need = cand && mhclust_find<MhcDev>(p.label, (int32_t)q) != mhclust_find<MhcDev>(p.label, f);
        const unsigned long long m = __ballot(need);
        const int n = __popcll(m);
        wave_handoff();                                         // the candidates of the turn before are read
        if (need) { const int at = (int)wv::mbcnt(m); s_q[wave][at] = (int32_t)q; s_f[wave][at] = f; }
        wave_handoff();
        for (int c0 = 0; c0 < n; c0 += per) {
            const int c = c0 + sub;
            const bool have = c < n;
            const int64_t qa = have ? s_q[wave][c] : 0, qc = have ? s_f[wave][c] : 0;
            int cnt = 0;
            for (int i0 = 0; i0 < H; i0 += S) {                 // (one round up to H = 64: the trip count is the wave's)
                const int i = i0 + l;
                const bool eq = have && i < H && p.sig[qa * H + i] == p.sig[qc * H + i];
                cnt += __popcll((__ballot(eq) >> (sub * S)) & slice);
            }
            if (have && l == 0 && cnt >= p.min_equal) mhclust_unite<MhcDev>(p.label, (int32_t)qa, (int32_t)qc);
        }
    }
    if (lane == 0 && ncand) atomicAdd(&p.counts[1], ncand);
}

__global__ __launch_bounds__(256) void k_mhc_flatten(MhclustParams p)
{
    const int lane = lane_id();
    const int64_t nwaves = (int64_t)gridDim.x * 4;
    unsigned long long nroots = 0;
    for (int64_t base = ((int64_t)blockIdx.x * 4 + wave_in_block()) * 64; base < p.nseq; base += nwaves * 64) {
        const int64_t q = base + lane;
        bool root = false;
        if (q < p.nseq) {
            const int32_t r = mhclust_find<MhcDev>(p.label, (int32_t)q);
            root = r == (int32_t)q;
            p.label[q] = r;                                     // (the root of q's tree: a valid parent for a find that still passes here)
            if (p.keep) p.keep[q] = root ? 1 : 0;
            atomicAdd(&p.sizes[r], 1);
        }
        nroots += (unsigned long long)__popcll(__ballot(root));
    }
    if (lane == 0 && nroots) atomicAdd(&p.counts[0], nroots);
}

__global__ __launch_bounds__(256) void k_mhc_sizes(MhclustParams p)
{
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < p.nseq; q += stride) p.size[q] = p.sizes[p.label[q]];
}

void launch_mhclust_begin(const MhclustParams &p, hipStream_t s) { hipLaunchKernelGGL(k_mhc_begin, dim3(rows_blocks(p.nseq)), dim3(256), 0, s, p); }

void launch_mhclust_band(const MhclustParams &p, int band, hipStream_t s)
{
    hipLaunchKernelGGL(k_mhc_clear, dim3(rows_blocks(p.T)), dim3(256), 0, s, p);
    hipLaunchKernelGGL(k_mhc_insert, dim3(rows_blocks(p.nseq)), dim3(256), 0, s, p, band);
    hipLaunchKernelGGL(k_mhc_link, dim3(rows_blocks(p.nseq)), dim3(256), 0, s, p, band);
}

void launch_mhclust_finish(const MhclustParams &p, hipStream_t s)
{
    hipLaunchKernelGGL(k_mhc_flatten, dim3(rows_blocks(p.nseq)), dim3(256), 0, s, p);
    if (p.size) hipLaunchKernelGGL(k_mhc_sizes, dim3(rows_blocks(p.nseq)), dim3(256), 0, s, p);
}

} // namespace bfa
