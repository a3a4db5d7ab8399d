// bf_kernels_mlm.hip -- rows that are already there -> masked ids and labels for masked-language-model pretraining (bf_mlm.h has the lane
// code: the generator, eligibility, units, the decision, the cap; include/blingfiretokdll_amd.h RowsMlmMaskBatchDevice and RowsMlmPredictionsBatchDevice
// are the specification).
//
//  k_rows_mlm<G, WW>  the partition of k_rows_span: G = span_group(row_len) lanes share a row (a wave, or a power-of-two slice of one for rows of
//                     at most 32 cells: 64 / G rows per wave), every wave makes the same number of rounds (a row past the end is a group that
//                     loads and stores nothing) and, inside a round, the same number of chunks: no cross-lane operation is divergent.  A row is
//                     walked in chunks of G cells in order, lane l takes cell j0 + l (coalesced dword loads and stores).
//     WW = false      token masking: a cell is its own unit, nothing crosses lanes, one Philox evaluation per eligible cell.
//     WW = true       whole words over a start plane and an end plane: the end and the "joins a unit" flag of cell j - 1 come one lane up (lane 0:
//                     the carry of the chunk before), the head of a cell's unit is an inclusive max-scan of (continues ? -1 : j) in log2 G
//                     steps, lanes still at -1 take the carried head, and the last lane's (end, joins, head) is the next chunk's carry.  At most
//                     two Philox evaluations per cell, one where the cell is its unit's head.
// No LDS, no atomics, no scratch; the status word is not touched (the call has cleared it).  In place (ids_out == rows): a lane reads its own
// cell of `rows` and nothing else of it before it writes that cell; what it needs of its neighbour comes from the planes.
//
//  k_rows_mlm_cap<G, WW, C>  the same partition with a cap of P predictions per row and the kept cells gathered (RowsMlmPredictionsBatchDevice is
//                     the specification).  Three phases per row, every one a walk over the row's chunks:
//     A               eligibility and heads as above; every eligible cell evaluates its head's draw and keeps ONE 64-bit word, the unit's key
//                     (W[3] << 32 | h) when the unit is selected and all ones otherwise; the selected cells are counted by ballot + popcount
//                     (the ballot masked to the group's lanes).  C > 0: the row has at most C chunks and the words stay in registers (the chunk
//                     loops are unrolled, so the array is indexed statically); C = 0: G = 64, rows of more than 256 cells, the words live in
//                     LDS, 8 bytes per cell in the wave's own slice, and a lane reads only what it wrote itself: no barrier.  A row of 4096
//                     cells takes 32 KiB, so the launcher sizes the block to at most 32 KiB of LDS: one wave per block there.
//     B               only in waves with a group whose count exceeds P (one vote, uniform per wave): T = max { t : #{key < t} <= P } from the
//                     high bit down, 32 + ceil(log2 row_len) rounds of a compare, a ballot and a popcount per chunk; the loop ends early once
//                     every such group of the wave sits at exactly P cells (no later bit can change who is kept).
//     C               kept = the row fits, or key < T; the slot of a kept cell is the popcount of the kept lanes below it plus the carry of
//                     the chunks before.  Only kept cells evaluate their own draw.  The cell's id is still in a register (C > 0) or the lane
//                     reads its own cell of `rows` again (C = 0), then writes ids, labels and the two gathered entries; the group fills the
//                     tail [n, P) and its lane 0 writes the count.
// No atomics, no scratch, the status word is not touched; the cross-lane operations (shuffles, ballots, the vote) are never under divergent
// control flow: the loop bounds depend on row_len and the wave's round alone.
#include "bf_kernels_common.h"

namespace bfa {

template <int G, bool WW>
__global__ __launch_bounds__(256) void k_rows_mlm(RowsMlmParams p)
{
    int64_t nrows = p.nrows ? *p.nrows : p.rows_cap;
    if (nrows > p.rows_cap) nrows = p.rows_cap;
    const int lane = threadIdx.x & (G - 1);
    const int64_t per_grid = (int64_t)gridDim.x * (256 / G);                       // rows per round of the grid
    const int64_t wave_row = ((int64_t)blockIdx.x * 256 + (threadIdx.x & ~63)) / G; // the first row of this wave's round
    for (int64_t r0 = wave_row; r0 < nrows; r0 += per_grid) {
        const int64_t r = r0 + (threadIdx.x & 63) / G;
        const bool live = r < nrows;
        const int64_t base = r * p.row_len;
        MlmCarry carry = mlm_carry_none();
        for (int j0 = 0; j0 < p.row_len; j0 += G) {
            const int j = j0 + lane;
            const bool in = live && j < p.row_len;
            int32_t id = 0, S = -1, E = 0;
            bool eligible = false;
            if (in) {
                const int64_t c = base + j;
                id = p.rows[c];
                eligible = mlm_eligible(p.spec, id, p.mask ? p.mask[c] : (uint8_t)1, p.seg ? p.seg[c] : 1);
                if (WW) { S = p.start_plane[c]; E = p.end_plane[c]; }
            }
            int h = j;
            if (WW) {
                const int joins = mlm_joins(eligible, S) ? 1 : 0;
                int32_t end_prev = __shfl_up(E, 1, G);
                int joins_prev = __shfl_up(joins, 1, G);
                if (lane == 0) { end_prev = carry.end; joins_prev = carry.joins; }
                h = mlm_head_seed(mlm_continues(joins_prev != 0, end_prev, joins != 0, S), j);
#pragma unroll
                for (int d = 1; d < G; d <<= 1) h = mlm_head_step(h, __shfl_up(h, d, G), lane >= d);
                h = mlm_head_close(h, carry.head);
                carry = MlmCarry{__shfl(E, G - 1, G), __shfl(joins, G - 1, G), __shfl(h, G - 1, G)};
            }
            if (in) {
                int32_t id_out, label;
                mlm_decide(p.spec, r, j, h, id, eligible, &id_out, &label);
                if (p.ids_out) p.ids_out[base + j] = id_out;
                if (p.labels_out) p.labels_out[base + j] = label;
            }
        }
    }
}

template <int G>
static void launch_rows_mlm_g(const RowsMlmParams &p, hipStream_t s)
{
    const int64_t rows = p.rows_cap < ((int64_t)1 << 40) ? p.rows_cap : ((int64_t)1 << 40);      // (the row count is on the device: the capacity bounds it)
    const dim3 grid(rows_blocks(rows * G));
    if (p.start_plane) hipLaunchKernelGGL((k_rows_mlm<G, true>), grid, dim3(256), 0, s, p);
    else hipLaunchKernelGGL((k_rows_mlm<G, false>), grid, dim3(256), 0, s, p);
}

// the words of a row's cells: registers (C chunks) or the wave's slice of LDS (C = 0)
template <int C> struct CapWords {
    uint64_t w[C]; int32_t ids[C];                      // (the cell's id stays too: phase C does not wait for a second load)
    __device__ __forceinline__ CapWords(uint64_t *, int) {}
    __device__ __forceinline__ void put(int c, uint64_t v, int32_t id) { w[c] = v; ids[c] = id; }
    __device__ __forceinline__ uint64_t get(int c) const { return w[c]; }
    __device__ __forceinline__ int32_t id(int c, const int32_t *) const { return ids[c]; }
};
template <> struct CapWords<0> {
    uint64_t *at;
    __device__ __forceinline__ CapWords(uint64_t *lds, int nchunks) : at(lds + (size_t)wave_in_block() * (size_t)nchunks * 64 + lane_id()) {}
    __device__ __forceinline__ void put(int c, uint64_t v, int32_t) { at[c * 64] = v; }
    __device__ __forceinline__ uint64_t get(int c) const { return at[c * 64]; }
    __device__ __forceinline__ int32_t id(int, const int32_t *cell) const { return *cell; }          // the lane's own cell of `rows`, not yet written
};

// one walk over a row's chunks: C > 0 unrolls C steps and skips those past the row (the same steps in every lane: row_len decides)
template <int C, class F> __device__ __forceinline__ void cap_chunks(int nchunks, F &&step)
{
    if constexpr (C > 0) {
#pragma unroll
        for (int c = 0; c < C; ++c) if (c < nchunks) step(c);
    } else {
        for (int c = 0; c < nchunks; ++c) step(c);
    }
}

template <int G, bool WW, int C>
__global__ __launch_bounds__(256) void k_rows_mlm_cap(RowsMlmCapParams q)
{
    extern __shared__ uint64_t cap_lds[];
    const RowsMlmParams &p = q.m;
    int64_t nrows = p.nrows ? *p.nrows : p.rows_cap;
    if (nrows > p.rows_cap) nrows = p.rows_cap;
    const int lane = threadIdx.x & (G - 1);
    const int shift = (int)(threadIdx.x & 63u) & ~(G - 1);                              // the group's first lane in the wave
    const uint64_t group = (G == 64 ? ~(uint64_t)0 : (((uint64_t)1 << G) - 1)) << shift;   // the group's lanes of a ballot
    const int nchunks = (p.row_len + G - 1) / G, P = q.max_pred;
    const int head_bits = mlm_cap_head_bits(p.row_len), rounds = mlm_cap_rounds(head_bits);
    CapWords<C> words(cap_lds, nchunks);
    const int64_t per_grid = (int64_t)gridDim.x * (blockDim.x / G);
    const int64_t wave_row = ((int64_t)blockIdx.x * blockDim.x + (threadIdx.x & ~63u)) / G;
    for (int64_t r0 = wave_row; r0 < nrows; r0 += per_grid) {
        const int64_t r = r0 + (threadIdx.x & 63) / G;
        const bool live = r < nrows;
        const int64_t base = r * p.row_len;
        // ---- A: the word of every cell, the selected cells of the row
        MlmCarry carry = mlm_carry_none();
        int selected = 0;
        cap_chunks<C>(nchunks, [&](int c) {
            const int j = c * G + lane;
            const bool in = live && j < p.row_len;
            int32_t id = 0, S = -1, E = 0;
            bool eligible = false;
            if (in) {
                const int64_t cell = base + j;
                id = p.rows[cell];
                eligible = mlm_eligible(p.spec, id, p.mask ? p.mask[cell] : (uint8_t)1, p.seg ? p.seg[cell] : 1);
                if (WW) { S = p.start_plane[cell]; E = p.end_plane[cell]; }
            }
            int h = j;
            if (WW) {
                const int joins = mlm_joins(eligible, S) ? 1 : 0;
                int32_t end_prev = __shfl_up(E, 1, G);
                int joins_prev = __shfl_up(joins, 1, G);
                if (lane == 0) { end_prev = carry.end; joins_prev = carry.joins; }
                h = mlm_head_seed(mlm_continues(joins_prev != 0, end_prev, joins != 0, S), j);
#pragma unroll
                for (int d = 1; d < G; d <<= 1) h = mlm_head_step(h, __shfl_up(h, d, G), lane >= d);
                h = mlm_head_close(h, carry.head);
                carry = MlmCarry{__shfl(E, G - 1, G), __shfl(joins, G - 1, G), __shfl(h, G - 1, G)};
            }
            uint64_t word = MLM_CAP_NONE;
            if (eligible) word = mlm_cap_word(p.spec, true, mlm_draw(p.spec, r, h), h);
            words.put(c, word, id);
            selected += mlm_popcount64(__ballot(word != MLM_CAP_NONE) & group);
        });
        // ---- B: the threshold, where a row of this wave does not fit
        uint64_t T = 0;
        if (__any(selected > P)) {
            bool settled = selected <= P;
            for (int i = rounds - 1; i >= 0; --i) {
                const uint64_t probe = mlm_cap_probe(T, i, head_bits);
                int n = 0;
                cap_chunks<C>(nchunks, [&](int c) { n += mlm_popcount64(__ballot(mlm_cap_below(words.get(c), probe)) & group); });
                T = mlm_cap_take(T, probe, n, P);
                settled = settled || n == P;                         // g(T) = P: no later bit changes who is kept
                if (__all(settled)) break;
            }
        }
        // ---- C: the cells, the gathered entries, the tail and the count
        MlmCapCarry slots = mlm_cap_carry_none();
        cap_chunks<C>(nchunks, [&](int c) {
            const int j = c * G + lane;
            const bool in = live && j < p.row_len;
            const bool kept = in && mlm_cap_kept(words.get(c), selected, P, T);
            const uint64_t kept_lanes = (__ballot(kept) & group) >> shift;
            if (in) {
                const int64_t cell = base + j;
                const int32_t id = words.id(c, p.rows + cell);
                const int32_t id_out = kept ? mlm_kept_id(p.spec, r, j, id) : id;
                if (p.ids_out) p.ids_out[cell] = id_out;
                if (p.labels_out) p.labels_out[cell] = kept ? id : p.spec.ignore_label;
                const int k = mlm_cap_slot(slots, kept_lanes, lane);
                if (kept && k < P) {                          // (k < P always: the kept cells of a row are at most P)
                    if (q.pred_cell) q.pred_cell[r * (int64_t)P + k] = j;
                    if (q.pred_label) q.pred_label[r * (int64_t)P + k] = id;
                }
            }
            slots = mlm_cap_carry_next(slots, kept_lanes);
        });
        if (live) {
            for (int k = slots.kept + lane; k < P; k += G) {
                if (q.pred_cell) q.pred_cell[r * (int64_t)P + k] = 0;
                if (q.pred_label) q.pred_label[r * (int64_t)P + k] = p.spec.ignore_label;
            }
            if (lane == 0 && q.pred_count) q.pred_count[r] = slots.kept;
        }
    }
}

template <int G, int C>
static void launch_rows_mlm_cap_g(const RowsMlmCapParams &q, hipStream_t s)
{
    const int64_t rows = q.m.rows_cap < ((int64_t)1 << 40) ? q.m.rows_cap : ((int64_t)1 << 40);
    unsigned block = 256, lds = 0;
    dim3 grid(rows_blocks(rows * G));
    if (C == 0) {                                                                    // G = 64: a wave per row, its words in LDS, at most 32 KiB per block
        const unsigned per_wave = (unsigned)((q.m.row_len + 63) / 64) * 64u * 8u;
        unsigned waves = (32u << 10) / per_wave;
        waves = waves < 1 ? 1 : waves > 4 ? 4 : waves;
        block = waves * 64; lds = waves * per_wave;
        int64_t blocks = (rows + waves - 1) / waves;
        const int64_t most = (int64_t)device_cus() * 8 * (4 / waves);
        grid = dim3((unsigned)(blocks > most ? most : blocks < 1 ? 1 : blocks));
    }
    if (q.m.start_plane) hipLaunchKernelGGL((k_rows_mlm_cap<G, true, C>), grid, dim3(block), lds, s, q);
    else hipLaunchKernelGGL((k_rows_mlm_cap<G, false, C>), grid, dim3(block), lds, s, q);
}

void launch_rows_mlm_cap(const RowsMlmCapParams &q, hipStream_t s)
{
    switch (span_group(q.m.row_len)) {
    case 1: launch_rows_mlm_cap_g<1, 1>(q, s); break;
    case 2: launch_rows_mlm_cap_g<2, 1>(q, s); break;
    case 4: launch_rows_mlm_cap_g<4, 1>(q, s); break;
    case 8: launch_rows_mlm_cap_g<8, 1>(q, s); break;
    case 16: launch_rows_mlm_cap_g<16, 1>(q, s); break;
    case 32: launch_rows_mlm_cap_g<32, 1>(q, s); break;
    default:
        if (q.m.row_len <= 64) launch_rows_mlm_cap_g<64, 1>(q, s);
        else if (q.m.row_len <= 128) launch_rows_mlm_cap_g<64, 2>(q, s);
        else if (q.m.row_len <= 256) launch_rows_mlm_cap_g<64, 4>(q, s);
        else launch_rows_mlm_cap_g<64, 0>(q, s);
        break;
    }
}

void launch_rows_mlm(const RowsMlmParams &p, hipStream_t s)
{
    switch (span_group(p.row_len)) {
    case 1: launch_rows_mlm_g<1>(p, s); break;
    case 2: launch_rows_mlm_g<2>(p, s); break;
    case 4: launch_rows_mlm_g<4>(p, s); break;
    case 8: launch_rows_mlm_g<8>(p, s); break;
    case 16: launch_rows_mlm_g<16>(p, s); break;
    case 32: launch_rows_mlm_g<32>(p, s); break;
    default: launch_rows_mlm_g<64>(p, s); break;
    }
}

} // namespace bfa
