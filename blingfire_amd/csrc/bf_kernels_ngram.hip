// bf_kernels_ngram.hip -- ragged ids -> a set of n-gram fingerprints in a caller-owned hash table, and the overlap of ragged ids with such a set
// (bf_ngram.h has the lane code, the specification and the split; include/blingfiretokdll_amd.h IdsToNgramSetBatchDevice is the contract).
//
//  k_ng_begin     the set call: its three counts to 0 and, with flags bit 0, the table to 0 (a lane per slot).
//  k_ng_lens      lane per sequence: a bad range is read as empty (status bit 3); its length; ngrams[q] when taken.
//  (scan)         k_scan_* of bf_kernels_sp.hip over the lengths -> W; T = W[nseq].
//  k_ng_init      lane per sequence: 0 into hits[q] and covered[q] of the rows that take atomic adds or that no lane meets (ngram_inside).
//  k_ng_tile<SET> persistent waves, a tile of NGRAM_TILE stream positions per wave and turn, 16 consecutive positions per lane.  The wave finds
//                 the sequences of the first and the last staged position by two searches of W (64 probes a round); a lane finds its own
//                 between them.  Then, with a hand-off between the passes: stage m(id) into the wave's skewed LDS block (own positions, one
//                 cell of each halo); 16 fingerprints per lane by Horner and roll; SET: insert them, three counts per wave, one 64-bit atomic
//                 add each; else: 16 home-slot loads at once, the collisions, the hit bits into the LDS bitmap, the left halo's starts probed
//                 by the lanes below n - 1, and the coverage windows, run counts and mask bytes of the lane's positions.
// Reads of ids and writes of the mask: cells off[q] + x with x < len[q] of a range that k_ng_lens has accepted, nothing else.  Table slots: below
// `slots`.  LDS: cells below NGRAM_STAGE (skewed: NGRAM_STAGE_QWORDS), bitmap words below NGRAM_BM_WORDS.
#include "bf_kernels_common.h"

namespace bfa {

// the memory policy of the device
struct NgramDev {
    static __device__ __forceinline__ uint64_t cas64(uint64_t *p, uint64_t expect, uint64_t v)
    {
        return (uint64_t)atomicCAS((unsigned long long *)p, (unsigned long long)expect, (unsigned long long)v);
    }
    static __device__ __forceinline__ void lds_or64(uint64_t *p, uint64_t v) { atomicOr((unsigned long long *)p, (unsigned long long)v); }
    static __device__ __forceinline__ void add32(int32_t *p, int32_t v) { atomicAdd(p, v); }
};

__global__ __launch_bounds__(256) void k_ng_begin(NgramParams p)
{
    const int64_t stride = (int64_t)gridDim.x * 256;
    if (blockIdx.x == 0 && threadIdx.x < 3) p.counts[threadIdx.x] = 0ull;
    if (p.clear) for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < p.slots; i += stride) p.table[i] = 0ull;
}

__global__ __launch_bounds__(256) void k_ng_lens(NgramParams p)
{
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < p.nseq; q += stride) {
        bool bad;
        const int32_t len = minhash_len(p.id_off[q], p.id_off[q + 1], p.ids_len, &bad);
        p.lens[q] = len;
        if (p.ngrams) p.ngrams[q] = ngram_count(len, p.n);
        if (bad) atomicOr(p.status, BF_STATUS_BAD_OFFSETS);
    }
}

__global__ __launch_bounds__(256) void k_ng_init(NgramParams p)
{
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < p.nseq; q += stride) {
        if (ngram_inside(p.W[q], p.W[q + 1])) continue;
        if (p.hits) p.hits[q] = 0;
        if (p.covered) p.covered[q] = 0;
    }
}

// the last q in [0, nseq) with W[q] <= t (t < W[nseq]), by the 64 lanes of the calling wave together; the answer is wave-uniform
__device__ __forceinline__ int64_t ng_find_seq(const int64_t *W, int64_t nseq, int64_t t)
{
    int64_t lo = 0, hi = nseq;
    const int lane = lane_id();
    while (hi - lo > 1) {
        const int64_t at = stream_probe(lo, hi, lane);
        const bool yes = at >= 0 && W[at] <= t;
        stream_narrow(&lo, &hi, __ballot(yes));
    }
    return lo;
}

// the sum of a small per-lane count over the wave, in every lane
__device__ __forceinline__ int ng_wave_sum(int v) { return __builtin_amdgcn_readlane(wv::incl_scan(v), 63); }

template <bool SET>
__global__ __launch_bounds__(256) void k_ng_tile(NgramParams p)
{
    __shared__ uint64_t s_m[4][NGRAM_STAGE_QWORDS];
    __shared__ uint64_t s_bm[4][NGRAM_BM_WORDS];
    const int lane = lane_id(), wave = wave_in_block();
    uint64_t *const sm = s_m[wave], *const bm = s_bm[wave];
    const int64_t T = p.W[p.nseq], ntiles = ngram_ntiles(T);
    unsigned long long wread = 0, wstored = 0, wfull = 0;       // SET: the wave's three counts (every lane holds the same numbers)
    for (int64_t tile = (int64_t)blockIdx.x * 4 + wave; tile < ntiles; tile += (int64_t)gridDim.x * 4) {
        NgramTile tl;
        tl.t0 = tile * NGRAM_TILE; tl.t1 = tl.t0 + NGRAM_TILE < T ? tl.t0 + NGRAM_TILE : T; tl.T = T; tl.n = p.n; tl.seed = p.seed; tl.bpow = p.bpow;
        const int64_t qa = ng_find_seq(p.W, p.nseq, SET ? tl.t0 : ngram_stage_lo(tl.t0, tl.n));
        const int64_t qe = ng_find_seq(p.W, p.nseq, ngram_stage_hi(tl.t1, T, tl.n) - 1);
        const StreamGlobal src{p.W, p.id_off, qa, qe, 0};
        wave_handoff();                                         // the tile before is read
        if (!SET && lane < NGRAM_BM_WORDS) bm[lane] = 0ull;
        StreamUnit first{0, 0, 0, 0};
        uint32_t vmask;
        ngram_stage_own(tl, src, p.ids, lane, sm, &first, &vmask);
        const int64_t tr = ngram_right_pos(tl, lane), tleft = SET ? -1 : ngram_left_pos(tl, lane);
        if (tr >= 0) ngram_stage_at(tl, src, p.ids, tr, ngram_pos_cell(tl, tr), sm);
        const bool left = tleft >= 0 && ngram_stage_at(tl, src, p.ids, tleft, ngram_pos_cell(tl, tleft), sm);
        wave_handoff();
        uint32_t hmask = 0;
        int nread = 0, nstored = 0, nfull = 0;                  // SET: the lane's counts of this tile, at most 16 each
        if (vmask) {
            uint64_t g[NGRAM_LANE];
            ngram_prints(tl, sm, lane, vmask, g);
            if (SET) {
#pragma unroll
                for (int k = 0; k < NGRAM_LANE; ++k) {
                    if (g[k] == 0ull) continue;
                    const int r = ngram_insert<NgramDev>(p.table, p.slots, g[k]);
                    ++nread; nstored += r == NGRAM_STORED; nfull += r == NGRAM_NO_SLOT;
                }
            } else {
                hmask = ngram_probe16(p.table, p.slots, g);
                ngram_put_hits<NgramDev>(bm, lane, hmask);
            }
        }
        if (SET) {
            wread += (unsigned long long)ng_wave_sum(nread); wstored += (unsigned long long)ng_wave_sum(nstored); wfull += (unsigned long long)ng_wave_sum(nfull);
        } else {
            if (left && ngram_lookup(p.table, p.slots, ngram_final(ngram_horner(sm, ngram_pos_cell(tl, tleft), tl.n), tl.n))) ngram_put_left<NgramDev>(tl, bm, tleft);
            wave_handoff();
            ngram_runs<NgramDev>(tl, src, first, lane, bm, hmask, p.hits, p.covered, p.mask);
        }
    }
    if (SET && lane == 0) {
        if (wread) atomicAdd(&p.counts[0], wread);
        if (wstored) atomicAdd(&p.counts[1], wstored);
        if (wfull) { atomicAdd(&p.counts[2], wfull); atomicOr(p.status, NGRAM_STATUS_FULL); }
    }
}

void launch_ngram_begin(const NgramParams &p, hipStream_t s)
{
    hipLaunchKernelGGL(k_ng_begin, dim3(rows_blocks(p.clear ? p.slots : 1)), dim3(256), 0, s, p);
}

void launch_ngram_lens(const NgramParams &p, hipStream_t s) { hipLaunchKernelGGL(k_ng_lens, dim3(rows_blocks(p.nseq)), dim3(256), 0, s, p); }

void launch_ngram_init(const NgramParams &p, hipStream_t s) { hipLaunchKernelGGL(k_ng_init, dim3(rows_blocks(p.nseq)), dim3(256), 0, s, p); }

template <bool SET> static void launch_tile(const NgramParams &p, hipStream_t s)
{
    static int per_cu = 0;
    if (per_cu <= 0) per_cu = resident_per_cu(k_ng_tile<SET>, 256, 0, 2);
    // T is known on the device alone (ranges may overlap): the grid comes from ids_len, the kernel strides over whatever tiles there are
    const int64_t need = (ngram_ntiles(p.ids_len) + 3) / 4;
    hipLaunchKernelGGL(k_ng_tile<SET>, dim3((unsigned)resident_blocks(per_cu, need)), dim3(256), 0, s, p);
}

void launch_ngram_set(const NgramParams &p, hipStream_t s) { launch_tile<true>(p, s); }
void launch_ngram_overlap(const NgramParams &p, hipStream_t s) { launch_tile<false>(p, s); }

} // namespace bfa
