// bf_kernels_mlm.hip -- rows that are already there -> masked ids and labels for masked-language-model pretraining (bf_mlm.h has the lane
// code: the generator, eligibility, units, the decision, the cap; include/blingfiretokdll_amd.h RowsMlmMaskBatchDevice and RowsMlmPredictionsBatchDevice
// are the specification).
//
//  k_rows_mlm<G, WW>  bf_rowwalk.h's partition (G lanes share a row, every wave the same rounds and, inside a round, the same chunks: no
//                     cross-lane operation is divergent).  A row is walked in chunks of G cells in order, lane l takes cell j0 + l.
//     WW = false      token masking: a cell is its own unit, nothing crosses lanes, one Philox evaluation per eligible cell.
//     WW = true       whole words over a start plane and an end plane: the head of a cell's unit comes from bf_rowwalk.h mlm_chunk_head, one
//                     scan per chunk with a carry between chunks.  At most two Philox evaluations per cell, one where the cell is its unit's head.
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
#include "bf_rowwalk.h"

namespace bfa {

template <int G, bool WW>
__global__ __launch_bounds__(256) void k_rows_mlm(RowsMlmParams p)
{
    const int64_t nrows = rows_bound(p.nrows, p.rows_cap);
    const int lane = group_lane<G>();
    for (int64_t step = rows_per_round<G>(256), r0 = wave_first_row<G>(256); r0 < nrows; r0 += step) {
        const int64_t r = group_row<G>(r0);
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
            if (WW) { const MlmHead m = mlm_chunk_head<G>(eligible, S, E, j, lane, carry); h = m.h; carry = m.carry; }
            if (in) {
                int32_t id_out, label;
                mlm_decide(p.spec, r, j, h, id, eligible, &id_out, &label);
                if (p.ids_out) p.ids_out[base + j] = id_out;
                if (p.labels_out) p.labels_out[base + j] = label;
            }
        }
    }
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
    const int64_t nrows = rows_bound(p.nrows, p.rows_cap);
    const int lane = group_lane<G>();
    const GroupBallot group_ballot = group_ballots<G>();
    const int nchunks = (p.row_len + G - 1) / G, P = q.max_pred;
    const int head_bits = mlm_cap_head_bits(p.row_len), rounds = mlm_cap_rounds(head_bits);
    CapWords<C> words(cap_lds, nchunks);
    for (int64_t step = rows_per_round<G>(blockDim.x), r0 = wave_first_row<G>(blockDim.x); r0 < nrows; r0 += step) {   // (the launcher sizes the block of the LDS form)
        const int64_t r = group_row<G>(r0);
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
            if (WW) { const MlmHead m = mlm_chunk_head<G>(eligible, S, E, j, lane, carry); h = m.h; carry = m.carry; }
            uint64_t word = MLM_CAP_NONE;
            if (eligible) word = mlm_cap_word(p.spec, true, mlm_draw(p.spec, r, h), h);
            words.put(c, word, id);
            selected += mlm_popcount64(group_ballot.in_place(word != MLM_CAP_NONE));
        });
        // ---- B: the threshold, where a row of this wave does not fit
        uint64_t T = 0;
        if (__any(selected > P)) {
            bool settled = selected <= P;
            for (int i = rounds - 1; i >= 0; --i) {
                const uint64_t probe = mlm_cap_probe(T, i, head_bits);
                int n = 0;
                cap_chunks<C>(nchunks, [&](int c) { n += mlm_popcount64(group_ballot.in_place(mlm_cap_below(words.get(c), probe))); });
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
            const uint64_t kept_lanes = group_ballot(kept);
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
    unsigned block = 256, lds = 0;
    dim3 grid(rows_grid(q.m.rows_cap, G));
    if (C == 0) {                                                                    // G = 64: a wave per row, its words in LDS, at most 32 KiB per block
        const unsigned per_wave = (unsigned)((q.m.row_len + 63) / 64) * 64u * 8u;
        unsigned waves = (32u << 10) / per_wave;
        waves = waves < 1 ? 1 : waves > 4 ? 4 : waves;
        block = waves * 64; lds = waves * per_wave;
        int64_t blocks = (rows_bounded(q.m.rows_cap) + waves - 1) / waves;
        const int64_t most = (int64_t)device_cus() * 8 * (4 / waves);
        grid = dim3((unsigned)(blocks > most ? most : blocks < 1 ? 1 : blocks));
    }
    if (q.m.start_plane) hipLaunchKernelGGL((k_rows_mlm_cap<G, true, C>), grid, dim3(block), lds, s, q);
    else hipLaunchKernelGGL((k_rows_mlm_cap<G, false, C>), grid, dim3(block), lds, s, q);
}

void launch_rows_mlm_cap(const RowsMlmCapParams &q, hipStream_t s)
{
    dispatch_span_group(q.m.row_len, [&](auto g) {
        constexpr int G = g();
        if constexpr (G < 64) launch_rows_mlm_cap_g<G, 1>(q, s);                      // (one chunk; a wave per row: its chunks decide where the words live)
        else if (q.m.row_len <= 64) launch_rows_mlm_cap_g<G, 1>(q, s);
        else if (q.m.row_len <= 128) launch_rows_mlm_cap_g<G, 2>(q, s);
        else if (q.m.row_len <= 256) launch_rows_mlm_cap_g<G, 4>(q, s);
        else launch_rows_mlm_cap_g<G, 0>(q, s);
    });
}

void launch_rows_mlm(const RowsMlmParams &p, hipStream_t s)
{
    dispatch_span_group(p.row_len, [&](auto g) {
        const dim3 grid(rows_grid(p.rows_cap, g()));
        if (p.start_plane) hipLaunchKernelGGL((k_rows_mlm<g(), true>), grid, dim3(256), 0, s, p);
        else hipLaunchKernelGGL((k_rows_mlm<g(), false>), grid, dim3(256), 0, s, p);
    });
}

} // namespace bfa
