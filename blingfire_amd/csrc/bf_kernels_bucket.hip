// bf_kernels_bucket.hip -- ragged ids -> length-bucketed batches: the units sorted by width (widest first, stable), the sorted list cut into
// batches under a cell budget, every batch padded to its own longest row (bf_bucket.h has the lane code and what a batch is;
// include/blingfiretokdll_amd.h IdsToBucketedRowsBatchDevice is the specification).
//
//  k_bucket_keys     lane per sequence: a range outside its array or with decreasing offsets is read as empty (status bit 3); key = max_len - width.
//  per pass of 8 bits (bucket_passes(max_len) of them, the host counts them from max_len alone), records = (key, value) in two arrays:
//    k_bucket_count    a block owns BUCKET_TILE consecutive records: a 256-bin histogram in LDS (atomics: a count does not depend on order), its
//                      column of the bin-major [256][nblocks] count array.
//    (scan)            k_scan_* of bf_kernels_sp.hip over that array -> the base of every (digit, block).
//    k_bucket_scatter  the same tile, wave w of the block its consecutive quarter, 64 records a round and in order.  The lanes of a round that hold
//                      one digit find each other by match-any -- eight ballots, each ANDed or AND-NOTed into the peer mask -- and a lane's rank
//                      is mbcnt(peers).  A first walk sums the populations into the wave's 256 counters in LDS (one lane per digit and round
//                      writes: no atomic); a prefix over the four waves on top of the block's base turns them into the wave's running offsets,
//                      which the second walk carries from round to round: position = offset[digit] + rank, then the lowest peer adds the
//                      population.  Keys and peer masks stay in registers between the walks (8 rounds: 24 registers).  Placement is ballots and
//                      prefix sums only, never the arrival order of an atomic: the sort is stable and the same from run to run.  The stores go
//                      straight to global memory: records of one digit and round are consecutive, and with one or two passes over widths most
//                      rounds hold few digits.  (No copy of the digit-sorted tile is staged in LDS.)  Pass 0 reads no values: the value is the index.
//  k_bucket_next     lane per sorted position: next(i) from the sorted width into the packed stage's jump array, mark = {0}; order and seq_pos.
//  k_packed_double   (bf_kernels_packed.hip, through its launcher) packed_rounds(nseq) rounds mark the batch starts.
//  (scan)            over the marks -> the batch of every position; the total is B.
//  k_bucket_first    lane per position: a marked position writes itself to first[its batch]; first[B] = nseq.
//  k_bucket_lens     lane per position: L of its batch (from the width at the batch's first position).
//  (scan)            over those L -> every position's first cell, C_b at a batch's first position, the cell total at nseq (bf_bucket.h bucket_cell).
//  k_bucket_batches  lane per position: batch_first, batch_len, batch_cell below batches_cap; the counts; status bit 0.
//  k_bucket_fill     a wave takes BUCKET_FILL_GROUP consecutive sorted positions, grid-stride.  Rows of more than 32 lanes take the wave one after
//                    the other; shorter ones -- the sorted tail, where most rows are -- share it in power-of-two slices (bucket_slice).  A lane
//                    writes four cells (16-byte rows store, 4-byte mask store: multiple % 4 == 0 and aligned planes) or one.  The ids of a row
//                    are read in order from ids[off[q] - lead + x]: coalesced.
#include "bf_kernels_common.h"

namespace bfa {

__global__ __launch_bounds__(256) void k_bucket_keys(BucketParams p)
{
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < p.nseq; q += stride) {
        bool bad;
        const int64_t n = rows_seq_len(p.id_off[q], p.id_off[q + 1], p.ids_len, &bad);
        p.key[0][q] = bucket_key(p.spec, packed_width(p.spec.unit, n));
        if (bad) atomicOr(p.status, BF_STATUS_BAD_OFFSETS);
    }
}

__global__ __launch_bounds__(BUCKET_THREADS) void k_bucket_count(BucketParams p, int pass)
{
    __shared__ uint32_t hist[BUCKET_BINS];
    const uint32_t *kin = p.key[pass & 1];
    hist[threadIdx.x] = 0;
    __syncthreads();
    const int64_t tile = (int64_t)blockIdx.x * BUCKET_TILE;
#pragma unroll
    for (int r = 0; r < BUCKET_TILE / BUCKET_THREADS; ++r) {
        const int64_t i = tile + r * BUCKET_THREADS + threadIdx.x;
        if (i < p.nseq) atomicAdd(&hist[bucket_digit(kin[i], pass)], 1u);
    }
    __syncthreads();
    p.counts[bucket_count_at(threadIdx.x, blockIdx.x, p.nblocks)] = (int32_t)hist[threadIdx.x];
}

__global__ __launch_bounds__(BUCKET_THREADS) void k_bucket_scatter(BucketParams p, int pass)
{
    __shared__ uint32_t off[BUCKET_WAVES][BUCKET_BINS];
    const int in = pass & 1;
    const uint32_t *kin = p.key[in];
    const int32_t *vin = p.val[in];
    uint32_t *kout = p.key[in ^ 1];
    int32_t *vout = p.val[in ^ 1];
    const int lane = lane_id(), wave = wave_in_block();
#pragma unroll
    for (int w = 0; w < BUCKET_WAVES; ++w) off[w][threadIdx.x] = 0;
    __syncthreads();
    const int64_t first = (int64_t)blockIdx.x * BUCKET_TILE + (int64_t)wave * BUCKET_WAVE_TILE + lane;
    uint32_t key[BUCKET_ROUNDS];
    unsigned long long peers[BUCKET_ROUNDS];
    // the first walk: every round's peer sets, their populations summed per digit
#pragma unroll
    for (int r = 0; r < BUCKET_ROUNDS; ++r) {
        const int64_t i = first + r * 64;
        const bool have = i < p.nseq;
        key[r] = have ? kin[i] : 0u;
        const uint32_t d = bucket_digit(key[r], pass);
        unsigned long long m = wv::ballot(have);
#pragma unroll
        for (int b = 0; b < BUCKET_RADIX_BITS; ++b) m = bucket_peers_step(m, wv::ballot(((d >> b) & 1u) != 0), d, b);
        peers[r] = m;
        if (have && bucket_leader(m, lane)) off[wave][d] += (uint32_t)__popcll(m);
        wave_handoff();
    }
    __syncthreads();
    // the digit of this thread: the block's base, then the waves in order
    {
        uint32_t base = (uint32_t)p.bases[bucket_count_at(threadIdx.x, blockIdx.x, p.nblocks)];
#pragma unroll
        for (int w = 0; w < BUCKET_WAVES; ++w) { const uint32_t c = off[w][threadIdx.x]; off[w][threadIdx.x] = base; base += c; }
    }
    __syncthreads();
    // the second walk: position = the wave's running offset of the digit + the rank among the round's peers
#pragma unroll
    for (int r = 0; r < BUCKET_ROUNDS; ++r) {
        const int64_t i = first + r * 64;
        const bool have = i < p.nseq;
        const uint32_t d = bucket_digit(key[r], pass);
        const uint32_t at = have ? off[wave][d] + wv::mbcnt(peers[r]) : 0u;
        wave_handoff();
        if (have && bucket_leader(peers[r], lane)) off[wave][d] += (uint32_t)__popcll(peers[r]);
        wave_handoff();
        if (have) {
            kout[at] = key[r];
            vout[at] = pass == 0 ? (int32_t)i : vin[i];
        }
    }
}

__global__ __launch_bounds__(256) void k_bucket_next(BucketParams p)
{
    const uint32_t *key = p.key[p.sorted];
    const int32_t *val = p.val[p.sorted];
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i <= p.nseq; i += stride) {
        p.jmp[0][i] = i < p.nseq ? bucket_next(p.spec, p.nseq, i, bucket_width(p.spec, key[i])) : (int32_t)p.nseq;
        p.mark[i] = i == 0 ? 1 : 0;
        if (i < p.nseq) {
            const int32_t q = val[i];
            if (p.order) p.order[i] = q;
            if (p.seq_pos) p.seq_pos[q] = (int32_t)i;
        }
    }
}

__global__ __launch_bounds__(256) void k_bucket_first(BucketParams p)
{
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i <= p.nseq; i += stride)
        if (i == p.nseq || p.mark[i]) p.first[p.mark_off[i]] = (int32_t)i;
}

__global__ __launch_bounds__(256) void k_bucket_lens(BucketParams p)
{
    const uint32_t *key = p.key[p.sorted];
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < p.nseq; i += stride)
        p.row_len[i] = bucket_row_len(p.spec, bucket_width(p.spec, key[p.first[p.mark_off[i] + p.mark[i] - 1]]));
}

__global__ __launch_bounds__(256) void k_bucket_batches(BucketParams p)
{
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i <= p.nseq; i += stride) {
        const bool end = i == p.nseq;
        if (!end && !p.mark[i]) continue;
        const int64_t b = p.mark_off[i], cell = p.row_cell[i];
        if (b <= p.batches_cap) {
            if (p.batch_first) p.batch_first[b] = (int32_t)i;
            if (p.batch_len) p.batch_len[b] = end ? 0 : p.row_len[i];
            if (p.batch_cell) p.batch_cell[b] = cell;
        }
        if (end) {
            p.counts_out[0] = b; p.counts_out[1] = cell;
            const bool lost_batches = b > p.batches_cap && (p.batch_first || p.batch_len || p.batch_cell);
            const bool lost_cells = cell > p.cells_cap && (p.rows || p.mask);
            if (lost_batches || lost_cells) atomicOr(p.status, 1);
        }
    }
}

// C cells per lane: 4 = the aligned form (every L is a multiple of 4, so is every row's first cell), 1 = any multiple and any base
template <int C>
__global__ __launch_bounds__(256) void k_bucket_fill(BucketParams p)
{
    const uint32_t *key = p.key[p.sorted];
    const int32_t *val = p.val[p.sorted];
    const PackedSpec &u = p.spec.unit;
    const int lane = lane_id();
    const int64_t ngroups = (p.nseq + BUCKET_FILL_GROUP - 1) / BUCKET_FILL_GROUP, nwaves = (int64_t)gridDim.x * 4;
    for (int64_t g = (int64_t)blockIdx.x * 4 + wave_in_block(); g < ngroups; g += nwaves) {
        const int64_t i0 = g * BUCKET_FILL_GROUP;
        const int n = (int)(p.nseq - i0 < BUCKET_FILL_GROUP ? p.nseq - i0 : BUCKET_FILL_GROUP);
        // the group's first row is its longest: the slice that holds it holds every row of the group
        const int S = bucket_slice(wv::uni(p.row_len[i0]) / C), per = 64 / S;
        const int sub = lane / S, x0 = (lane & (S - 1)) * C;
        for (int r0 = 0; r0 < n; r0 += per) {
            const int r = r0 + sub;
            if (r >= n) continue;
            const int64_t i = i0 + r;
            const int32_t w = bucket_width(p.spec, key[i]), L = p.row_len[i];
            const int64_t row = p.row_cell[i], src = p.id_off[val[i]] - u.lead;
            for (int32_t x = x0; x < L; x += S * C) {
                int32_t id[C]; uint8_t m[C];
#pragma unroll
                for (int k = 0; k < C; ++k) {
                    const int kind = bucket_cell_kind(u, w, x + k);
                    m[k] = kind != BUCKET_CELL_PAD;
                    id[k] = kind == BUCKET_CELL_ID ? p.ids[src + x + k] : kind == BUCKET_CELL_CLS ? u.cls_id : kind == BUCKET_CELL_SEP ? u.sep_id : u.pad_id;
                }
                const int64_t at = bucket_cell(row, x);
                if constexpr (C == 4) {
                    if (at + 4 <= p.cells_cap) {
                        if (p.rows) *(int4 *)(p.rows + at) = make_int4(id[0], id[1], id[2], id[3]);
                        if (p.mask) *(uint32_t *)(p.mask + at) = (uint32_t)m[0] | (uint32_t)m[1] << 8 | (uint32_t)m[2] << 16 | (uint32_t)m[3] << 24;
                        continue;
                    }
                }
#pragma unroll
                for (int k = 0; k < C; ++k) {
                    if (at + k >= p.cells_cap) break;
                    if (p.rows) p.rows[at + k] = id[k];
                    if (p.mask) p.mask[at + k] = m[k];
                }
            }
        }
    }
}

void launch_bucket_keys(const BucketParams &p, hipStream_t s) { hipLaunchKernelGGL(k_bucket_keys, dim3(rows_blocks(p.nseq)), dim3(256), 0, s, p); }
void launch_bucket_count(const BucketParams &p, int pass, hipStream_t s)
{
    hipLaunchKernelGGL(k_bucket_count, dim3((unsigned)p.nblocks), dim3(BUCKET_THREADS), 0, s, p, pass);
}
void launch_bucket_scatter(const BucketParams &p, int pass, hipStream_t s)
{
    hipLaunchKernelGGL(k_bucket_scatter, dim3((unsigned)p.nblocks), dim3(BUCKET_THREADS), 0, s, p, pass);
}
void launch_bucket_next(const BucketParams &p, hipStream_t s) { hipLaunchKernelGGL(k_bucket_next, dim3(rows_blocks(p.nseq + 1)), dim3(256), 0, s, p); }
void launch_bucket_first(const BucketParams &p, hipStream_t s) { hipLaunchKernelGGL(k_bucket_first, dim3(rows_blocks(p.nseq + 1)), dim3(256), 0, s, p); }
void launch_bucket_lens(const BucketParams &p, hipStream_t s) { hipLaunchKernelGGL(k_bucket_lens, dim3(rows_blocks(p.nseq)), dim3(256), 0, s, p); }
void launch_bucket_batches(const BucketParams &p, hipStream_t s) { hipLaunchKernelGGL(k_bucket_batches, dim3(rows_blocks(p.nseq + 1)), dim3(256), 0, s, p); }

void launch_bucket_fill(const BucketParams &p, hipStream_t s)
{
    const bool wide = p.spec.multiple % 4 == 0 && ((uintptr_t)p.rows & 15) == 0 && ((uintptr_t)p.mask & 3) == 0;
    const int64_t groups = (p.nseq + BUCKET_FILL_GROUP - 1) / BUCKET_FILL_GROUP;
    if (wide) hipLaunchKernelGGL(k_bucket_fill<4>, dim3(rows_blocks(groups * 64)), dim3(256), 0, s, p);
    else hipLaunchKernelGGL(k_bucket_fill<1>, dim3(rows_blocks(groups * 64)), dim3(256), 0, s, p);
}

} // namespace bfa
