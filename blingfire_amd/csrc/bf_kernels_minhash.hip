// bf_kernels_minhash.hip -- ragged ids -> MinHash signatures over shingles of ids, LSH band keys, and the equal-slot count of candidate pairs
// (bf_minhash.h has the lane code, the specification and the split; include/blingfiretokdll_amd.h IdsToMinHashBatchDevice is the contract).
//
//  k_mh_params   a lane per permutation: a_i, b_i from Philox into the workspace, once per call (not 40 Philox rounds per sequence).
//  k_mh_lens     lane per sequence: a range outside its array or with decreasing offsets is read as empty (status bit 3); its length, its
//                shingle count; status bit 0 when signatures are taken and nseq > sig_cap.
//  (scan)        k_scan_* of bf_kernels_sp.hip over the lengths -> W; T = W[nseq], the length of the stream of all ids laid end to end.
//  k_mh_init     a lane looks at one sequence, the wave then writes the all-ones row of each that needs one: the empty sequences, which no
//                tile meets, and those that span a tile's edge, whose row takes atomic mins (minhash_init_row).  It stores constants: idempotent.
//  k_mh_sig<NP>  persistent waves, a tile of MINHASH_TILE stream positions per wave and turn.  Lane l owns the permutations l, l + 64, ...
//                (NP = ceil(H / 64) of them: a, b and the minimum, 5 registers each, loaded once per wave).  The tile's first sequence comes
//                from the wave's search of W (stream_probe / stream_narrow); 64 consecutive sequences (W, length, offset: one per lane) are a
//                window the wave steps through with readlane, skipping empty ones by a ballot; a window without a further non-empty
//                sequence is left by another search, so a run of empty sequences costs one search, not a walk.  Per sequence and chunk of
//                64 shingle starts: the chunk's ids and the k - 1 behind them go to the wave's LDS slot with coalesced loads, lane j hashes
//                the shingle at start j from LDS, then the wave steps through the hashes -- each read with readlane into a scalar register,
//                so the multiply takes a scalar operand -- and every lane does a 64 x 32 multiply-add and a min per permutation it owns.
//                No cross-lane reduction anywhere.  At the sequence's end (or the tile's) the row goes out coalesced: a plain store for a
//                sequence inside the tile, atomicMin for one that spans an edge.  min is associative and commutative, so the bytes are the
//                same from run to run and for every grid size.
//  k_mh_bands    a lane per (sequence, band) over the finished signatures.
//  k_mh_pairs    a wave -- for H <= 32 a power-of-two slice of one -- compares the two rows of a pair; ballot and popcount give the count.
// Reads of ids: positions off[q] + x with x < n_q of a range that k_mh_lens has accepted, nothing else.
#include "bf_kernels_common.h"

namespace bfa {

__global__ __launch_bounds__(256) void k_mh_params(MinhashParams p)
{
    const int i = (int)threadIdx.x;
    if (i >= p.spec.H) return;
    const MinhashPerm m = minhash_perm(p.spec.seed, i);
    ((uint4 *)p.ab)[i] = make_uint4((uint32_t)m.a, (uint32_t)(m.a >> 32), (uint32_t)m.b, (uint32_t)(m.b >> 32));
}

__global__ __launch_bounds__(256) void k_mh_lens(MinhashParams p)
{
    const int64_t stride = (int64_t)gridDim.x * 256;
    if (blockIdx.x == 0 && threadIdx.x == 0 && p.sig && p.nseq > p.sig_cap) atomicOr(p.status, MINHASH_STATUS_CAP);
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < p.nseq; q += stride) {
        bool bad;
        const int32_t n = minhash_len(p.id_off[q], p.id_off[q + 1], p.ids_len, &bad);
        p.lens[q] = n;
        if (p.nshingles) p.nshingles[q] = minhash_nshingles(n, p.spec.k);
        if (bad) atomicOr(p.status, BF_STATUS_BAD_OFFSETS);
    }
}

__global__ __launch_bounds__(256) void k_mh_init(MinhashParams p)
{
    const int lane = lane_id(), H = p.spec.H;
    const int64_t rows = p.nseq < p.sig_cap ? p.nseq : p.sig_cap, nwaves = (int64_t)gridDim.x * 4;
    for (int64_t base = ((int64_t)blockIdx.x * 4 + wave_in_block()) * 64; base < rows; base += nwaves * 64) {
        const int64_t q = base + lane;
        unsigned long long m = __ballot(q < rows && minhash_init_row(p.W[q < rows ? q : 0], p.W[q < rows ? q + 1 : 0]));
        for (; m; m &= m - 1) {
            uint32_t *row = p.sig + (base + __builtin_ctzll(m)) * H;
            for (int i = lane; i < H; i += 64) row[i] = MINHASH_EMPTY;
        }
    }
}

// the last q in [0, nseq) with W[q] <= t (t < W[nseq]), by the 64 lanes of the calling wave together; the answer is wave-uniform
__device__ __forceinline__ int64_t mh_find_seq(const int64_t *W, int64_t nseq, int64_t t)
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

template <int NP>
__global__ __launch_bounds__(256) void k_mh_sig(MinhashParams p)
{
    __shared__ int32_t s_ids[4][MINHASH_CHUNK + MINHASH_MAX_SHINGLE];
    const int lane = lane_id(), wave = wave_in_block();
    const int k = p.spec.k, H = p.spec.H;
    const int64_t nseq = p.nseq;
    const int64_t T = p.W[nseq], ntiles = minhash_ntiles(T);
    const int64_t rows = nseq < p.sig_cap ? nseq : p.sig_cap;
    const uint32_t seed32 = minhash_seed32(p.spec.seed);
    int32_t *const s = s_ids[wave];
    uint64_t a[NP], b[NP];
    uint32_t mn[NP];
#pragma unroll
    for (int e = 0; e < NP; ++e) {
        const int i = lane + 64 * e;
        const uint4 w = i < H ? ((const uint4 *)p.ab)[i] : make_uint4(1u, 0u, 0u, 0u);
        a[e] = ((uint64_t)w.y << 32) | w.x; b[e] = ((uint64_t)w.w << 32) | w.z;
        mn[e] = MINHASH_EMPTY;
    }
    for (int64_t tile = (int64_t)blockIdx.x * 4 + wave; tile < ntiles; tile += (int64_t)gridDim.x * 4) {
        const int64_t t0 = tile * MINHASH_TILE, t1 = t0 + MINHASH_TILE < T ? t0 + MINHASH_TILE : T;
        // the window: 64 consecutive sequences from the one that holds t0, one per lane
        int64_t qb = mh_find_seq(p.W, nseq, t0), w_l = 0, o_l = 0;
        int32_t n_l = 0;
        int wi = 0;                                             // the sequence at hand is qb + wi; wi == 0: the window is loaded from qb
        for (;;) {
            if (wi == 0) {
                const int64_t qi = qb + lane;
                const bool have = qi < nseq;
                w_l = have ? p.W[qi] : T; n_l = have ? p.lens[qi] : 0; o_l = have ? p.id_off[qi] : 0;
            }
            const int64_t q = qb + wi, w0 = wv::bcast(w_l, wi), o = wv::bcast(o_l, wi);
            const int32_t n = wv::bcast(n_l, wi);
            if (n <= 0) break;                                  // (the search and the ballot below name non-empty sequences only)
            int32_t x0, x1;
            minhash_starts(w0, n, k, t0, &x0, &x1);
            const int32_t *src = p.ids + o;
            const int kk = minhash_width(n, k);
            for (int32_t c = x0; c < x1; c += MINHASH_CHUNK) {
                const int cnt = x1 - c < MINHASH_CHUNK ? x1 - c : MINHASH_CHUNK;
                const int need = cnt + kk - 1;                  // ids c .. c + need - 1 < n, at most CHUNK + MAX_SHINGLE - 1 of them
                wave_handoff();                                 // the chunk before is read
                if (lane < need) s[lane] = src[c + lane];
                if (lane + 64 < need) s[lane + 64] = src[c + 64 + lane];
                wave_handoff();
                uint32_t hsh = seed32;
                for (int i = 0; i < kk; ++i) hsh = minhash_step(hsh, s[lane + i]);      // (lanes >= cnt hash what lies there: never read below)
                // the walk: four hashes a turn (independent multiply-adds in flight), each a scalar operand
                auto take = [&](uint32_t sh) {
#pragma unroll
                    for (int e = 0; e < NP; ++e) {
                        const uint32_t v = minhash_hash(a[e], b[e], sh);
                        mn[e] = v < mn[e] ? v : mn[e];
                    }
                };
                int j = 0;
                for (; j + 4 <= cnt; j += 4) {
                    const uint32_t s0 = wv::bcast(hsh, j), s1 = wv::bcast(hsh, j + 1), s2 = wv::bcast(hsh, j + 2), s3 = wv::bcast(hsh, j + 3);
                    take(s0); take(s1); take(s2); take(s3);
                }
                for (; j < cnt; ++j) take(wv::bcast(hsh, j));
            }
            const int64_t w1 = w0 + n;
            if (x1 > x0) {
                const bool inside = minhash_inside(w0, w1);
#pragma unroll
                for (int e = 0; e < NP; ++e) {
                    const int i = lane + 64 * e;
                    if (i < H && q < rows) {
                        uint32_t *at = p.sig + q * H + i;
                        if (inside) *at = mn[e]; else atomicMin(at, mn[e]);
                    }
                    mn[e] = MINHASH_EMPTY;
                }
            }
            if (w1 >= t1) break;
            // the next non-empty sequence: in the window behind wi, else where the stream goes on
            const unsigned long long m = __ballot(n_l > 0) & ~((2ull << wi) - 1ull);
            if (m) wi = __builtin_ctzll(m);
            else { qb = mh_find_seq(p.W, nseq, w1); wi = 0; }
        }
    }
}

__global__ __launch_bounds__(256) void k_mh_bands(MinhashParams p)
{
    const int H = p.spec.H, r = p.spec.r, B = p.spec.B;
    const int64_t rows = p.nseq < p.sig_cap ? p.nseq : p.sig_cap, cells = rows * B, stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < cells; i += stride) {
        const int64_t q = i / B;
        const int band = (int)(i - q * B);
        p.keys[i] = (int64_t)minhash_band_key(p.spec.seed, band, p.sig + q * H + band * r, r);
    }
}

__global__ __launch_bounds__(256) void k_mh_pairs(MinhashPairsParams p)
{
    const int lane = lane_id(), H = p.H;
    const int S = minhash_pair_slice(H), per = 64 / S, sub = lane / S, l = lane & (S - 1);
    const unsigned long long slice = S == 64 ? ~0ull : ((1ull << S) - 1ull);
    const int64_t nwaves = (int64_t)gridDim.x * 4;
    for (int64_t base = ((int64_t)blockIdx.x * 4 + wave_in_block()) * per; base < p.npairs; base += nwaves * per) {
        const int64_t pi = base + sub;
        const bool have = pi < p.npairs;
        const int64_t qa = have ? p.pairs[2 * pi] : 0, qc = have ? p.pairs[2 * pi + 1] : 0;
        const bool ok = have && qa >= 0 && qa < p.nseq && qc >= 0 && qc < p.nseq;
        int cnt = 0;
        for (int i0 = 0; i0 < H; i0 += S) {                      // (one round up to H = 64: the trip count is the wave's)
            const int i = i0 + l;
            const bool eq = ok && i < H && p.sig[qa * H + i] == p.sig[qc * H + i];
            cnt += __popcll((__ballot(eq) >> (sub * S)) & slice);
        }
        if (have && l == 0) {
            p.equal[pi] = ok ? cnt : -1;
            if (!ok) atomicOr(p.status, BF_STATUS_BAD_OFFSETS);
        }
    }
}

void launch_minhash_prepare(const MinhashParams &p, hipStream_t s)
{
    hipLaunchKernelGGL(k_mh_params, dim3(1), dim3(256), 0, s, p);
    hipLaunchKernelGGL(k_mh_lens, dim3(rows_blocks(p.nseq)), dim3(256), 0, s, p);
}

void launch_minhash_init(const MinhashParams &p, hipStream_t s)
{
    const int64_t rows = p.nseq < p.sig_cap ? p.nseq : p.sig_cap;
    hipLaunchKernelGGL(k_mh_init, dim3(rows_blocks(rows)), dim3(256), 0, s, p);
}

template <int NP> static void launch_sig(const MinhashParams &p, hipStream_t s)
{
    static int per_cu = 0;
    if (per_cu <= 0) per_cu = resident_per_cu(k_mh_sig<NP>, 256, 0, 8);
    // T is known on the device alone (ranges may overlap): the grid comes from ids_len, the kernel strides over whatever tiles there are
    const int64_t need = (minhash_ntiles(p.ids_len) + 3) / 4;
    hipLaunchKernelGGL(k_mh_sig<NP>, dim3((unsigned)resident_blocks(per_cu, need)), dim3(256), 0, s, p);
}

void launch_minhash_sig(const MinhashParams &p, hipStream_t s)
{
    switch ((p.spec.H + 63) / 64) {
    case 1: launch_sig<1>(p, s); break;
    case 2: launch_sig<2>(p, s); break;
    case 3: launch_sig<3>(p, s); break;
    default: launch_sig<4>(p, s); break;
    }
}

void launch_minhash_bands(const MinhashParams &p, hipStream_t s)
{
    const int64_t rows = p.nseq < p.sig_cap ? p.nseq : p.sig_cap;
    hipLaunchKernelGGL(k_mh_bands, dim3(rows_blocks(rows * p.spec.B)), dim3(256), 0, s, p);
}

void launch_minhash_pairs(const MinhashPairsParams &p, hipStream_t s)
{
    const int per = 64 / minhash_pair_slice(p.H);
    hipLaunchKernelGGL(k_mh_pairs, dim3(rows_blocks((p.npairs + per - 1) / per * 64)), dim3(256), 0, s, p);
}

} // namespace bfa
