// bf_kernels_rows.hip -- ragged ids -> fixed-shape model inputs: the row stage (bf_rowstage_body.h has the kernels) over RowsSource (bf_rows.h has
// the cell logic and what a row is), the grid size every row-stage launch takes, and the span cells of rows that are already there (k_rows_span, over bf_rowwalk.h's partition).
#include "bf_rowstage_body.h"
#include "bf_rowwalk.h"

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

// RowsSpanCellsBatchDevice: bf_rowwalk.h's partition (G lanes share a row).  Lane l reads cells l, l + G, ... of both planes (coalesced: neighbouring
// lanes, neighbouring cells), keeps its best candidates (bf_rows.h span_cell / span_combine), the group reduces them by xor shuffles inside its
// slice -- no atomics, no LDS -- and its lane 0 writes the two cells.
template <int G>
__global__ __launch_bounds__(256) void k_rows_span(RowsSpanParams p)
{
    const int64_t nrows = rows_bound(p.nrows, p.rows_cap);
    const int lane = group_lane<G>();
    for (int64_t step = rows_per_round<G>(256), r0 = wave_first_row<G>(256); r0 < nrows; r0 += step) {
        const int64_t r = group_row<G>(r0);
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

void launch_rows_span(const RowsSpanParams &p, hipStream_t s)
{
    dispatch_span_group(p.row_len, [&](auto g) { hipLaunchKernelGGL(k_rows_span<g()>, dim3(rows_grid(p.rows_cap, g())), dim3(256), 0, s, p); });
}

} // namespace bfa
