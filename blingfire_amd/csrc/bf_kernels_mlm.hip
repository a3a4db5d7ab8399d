// bf_kernels_mlm.hip -- rows that are already there -> masked ids and labels for masked-language-model pretraining (bf_mlm.h has the lane
// code: the generator, eligibility, units, the decision; include/blingfiretokdll_amd.h RowsMlmMaskBatchDevice is the specification).
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
