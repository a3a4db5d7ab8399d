// bf_kernels_rows.hip -- ragged ids -> fixed-shape model inputs: the row stage (bf_rowstage_body.h has the kernels) over RowsSource (bf_rows.h has
// the cell logic and what a row is), the grid size every row-stage launch takes, and the span cells of rows that are already there (k_rows_span).
#include "bf_rowstage_body.h"

namespace bfa {

unsigned rows_blocks(int64_t items)
{
    int64_t blocks = (items + 255) / 256;
    if (blocks > (int64_t)device_cus() * 8) blocks = (int64_t)device_cus() * 8;
    return (unsigned)(blocks < 1 ? 1 : blocks);
}

template void launch_rowstage_count<RowsSource>(const RowStageParams<RowsSource> &p, hipStream_t s);
template void launch_rowstage_map<RowsSource>(const RowStageParams<RowsSource> &p, hipStream_t s);
template void launch_rowstage_fill<RowsSource>(const RowStageParams<RowsSource> &p, hipStream_t s);
template void launch_rowstage_planes<RowsSource>(const RowPlanesParams<RowsSource> &p, hipStream_t s);

// RowsSpanCellsBatchDevice: G = span_group(row_len) lanes share a row (a wave, or a power-of-two slice of one for rows of at most 32 cells: 64 / G rows
// per wave).  Lane l reads cells l, l + G, ... of both planes (coalesced: neighbouring lanes, neighbouring cells), keeps its best candidates
// (bf_rows.h span_cell / span_combine), the group reduces them by xor shuffles inside its slice -- no atomics, no LDS -- and its lane 0 writes the
// two cells.  Every wave makes the same number of rounds (a row past the end is a group that loads nothing): the shuffles are never divergent.
template <int G>
__global__ __launch_bounds__(256) void k_rows_span(RowsSpanParams p)
{
    int64_t nrows = p.nrows ? *p.nrows : p.rows_cap;
    if (nrows > p.rows_cap) nrows = p.rows_cap;
    const int lane = threadIdx.x & (G - 1);
    const int64_t per_grid = (int64_t)gridDim.x * (256 / G);                       // rows per round of the grid
    const int64_t wave_row = ((int64_t)blockIdx.x * 256 + (threadIdx.x & ~63)) / G; // the first row of this wave's round
    for (int64_t r0 = wave_row; r0 < nrows; r0 += per_grid) {
        const int64_t r = r0 + (threadIdx.x & 63) / G;
        const bool live = r < nrows;
        int64_t q = 0;
        bool known = false;
        if (live) { q = p.row_seq ? (int64_t)p.row_seq[r] : r; known = q >= 0 && q < p.nseq; }
        const int32_t a = known ? p.span_first[q] : -1, z = known ? p.span_last[q] : -1;
        SpanAcc acc = span_none();
        if (known && a >= 0 && z >= a) {
            const int32_t *S = p.start_plane + r * p.row_len, *E = p.end_plane + r * p.row_len;
            for (int j = lane; j < p.row_len; j += G) acc = span_combine(acc, span_cell(S[j], E[j], a, z, j));
        }
#pragma unroll
        for (int m = G / 2; m > 0; m >>= 1) acc = span_combine(acc, SpanAcc{__shfl_xor(acc.start, m, G), __shfl_xor(acc.end, m, G)});
        if (live && lane == 0) {
            span_result(acc, a, z, p.none_cell, &p.start_cell[r], &p.end_cell[r]);
            if (!known) atomicOr(p.status, BF_STATUS_BAD_OFFSETS);
        }
    }
}

template <int G>
static void launch_rows_span_g(const RowsSpanParams &p, hipStream_t s)
{
    const int64_t rows = p.rows_cap < ((int64_t)1 << 40) ? p.rows_cap : ((int64_t)1 << 40);      // (the row count is on the device: the capacity bounds it)
    hipLaunchKernelGGL(k_rows_span<G>, dim3(rows_blocks(rows * G)), dim3(256), 0, s, p);
}

void launch_rows_span(const RowsSpanParams &p, hipStream_t s)
{
    switch (span_group(p.row_len)) {
    case 1: launch_rows_span_g<1>(p, s); break;
    case 2: launch_rows_span_g<2>(p, s); break;
    case 4: launch_rows_span_g<4>(p, s); break;
    case 8: launch_rows_span_g<8>(p, s); break;
    case 16: launch_rows_span_g<16>(p, s); break;
    case 32: launch_rows_span_g<32>(p, s); break;
    default: launch_rows_span_g<64>(p, s); break;
    }
}

} // namespace bfa
