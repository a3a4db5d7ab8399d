// bf_kernels_rows.hip -- ragged ids -> fixed-shape model inputs (bf_rows.h has the cell logic and what a row is).
//
//  k_rows_count  lane per sequence: a range outside [0, ids_len] or with decreasing offsets counts as empty (status bit 3); windows -> counts.
//  (scan)        k_scan_* of bf_kernels_sp.hip over the counts -> row offsets; the row total stays on the device.
//  k_rows_map    lane per row below min(total, rows_cap): its sequence by binary search of the row offsets, the index of its first id (saturating
//                at INT32_MAX); rows beyond rows_cap, and a saturated index, are reported (status bit 0).
//  k_rows_fill   lane per four cells (row_len % 4 == 0 and both outputs aligned: one 16-byte store of ids, one 4-byte store of mask) or
//                per cell, over the flat cell space min(total, rows_cap) x row_len.  Ids are read with plain dword loads: a sequence
//                starts anywhere.
// No lane walks a sequence's windows or a row's cells: one sequence of 10^5 windows is 10^5 rows like any others.
#include "bf_kernels_common.h"
#include "bf_rows.h"

namespace bfa {

__global__ __launch_bounds__(256) void k_rows_count(RowsParams p)
{
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < p.nseq; q += stride) {
        bool bad, sat;
        const int64_t n = rows_seq_len(p.id_off[q], p.id_off[q + 1], p.ids_len, &bad);
        p.counts[q] = rows_count(p.spec, n, &sat);
        if (bad) atomicOr(p.status, BF_STATUS_BAD_OFFSETS);
        if (sat) atomicOr(p.status, 1);
    }
}

__global__ __launch_bounds__(256) void k_rows_map(RowsParams p)
{
    const int64_t total = p.row_off[p.nseq], nrows = total < p.rows_cap ? total : p.rows_cap;
    const int64_t stride = (int64_t)gridDim.x * 256, r0 = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r0 == 0 && total > p.rows_cap) atomicOr(p.status, 1);
    for (int64_t r = r0; r < nrows; r += stride) {
        const int64_t q = rows_find_seq(p.row_off, p.nseq, r);
        if (r < p.seq_rows) p.row_seq[r] = (int32_t)q;
        bool sat;
        const int32_t first = rows_first_i32((r - p.row_off[q]) * p.spec.step, &sat);
        if (r < p.first_rows) p.row_first[r] = first;
        if (sat) atomicOr(p.status, 1);
    }
}

// W cells per lane: 4 = the aligned form, 1 = any row_len and any base
template <int W>
__global__ __launch_bounds__(256) void k_rows_fill(RowsParams p)
{
    const int64_t total = p.row_off[p.nseq], nrows = total < p.rows_cap ? total : p.rows_cap;
    const int lw = p.spec.row_len / W;                                  // lanes per row
    const int64_t nlanes = nrows * lw, stride = (int64_t)gridDim.x * 256;
    int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nlanes) return;
    // the lane's (row, place in the row) moves by a fixed step from one round to the next: one division per lane, none per round
    int64_t r = i / lw;
    int jw = (int)(i - r * lw);
    const int64_t dr = stride / lw;
    const int dj = (int)(stride - dr * lw);
    for (;;) {
        const int64_t q = r < p.seq_rows ? (int64_t)p.row_seq[r] : rows_find_seq(p.row_off, p.nseq, r);
        int64_t first = r < p.first_rows ? (int64_t)p.row_first[r] : 0x7fffffff;
        if (first == 0x7fffffff) first = (r - p.row_off[q]) * p.spec.step;       // not held, or saturated: from the offsets
        bool bad;
        const int64_t b = p.id_off[q], n = rows_seq_len(b, p.id_off[q + 1], p.ids_len, &bad);
        const int32_t *seq = p.ids + (bad ? 0 : b);
        int32_t v[W]; uint8_t m[W];
#pragma unroll
        for (int k = 0; k < W; ++k) v[k] = rows_cell_value(p.spec, rows_cell(p.spec, first, n, jw * W + k), seq, &m[k]);
        const int64_t at = r * p.spec.row_len + (int64_t)jw * W;
        if constexpr (W == 4) {
            if (p.rows) *(int4 *)(p.rows + at) = make_int4(v[0], v[1], v[2], v[3]);
            if (p.mask) *(uint32_t *)(p.mask + at) = (uint32_t)m[0] | ((uint32_t)m[1] << 8) | ((uint32_t)m[2] << 16) | ((uint32_t)m[3] << 24);
        } else {
            if (p.rows) p.rows[at] = v[0];
            if (p.mask) p.mask[at] = m[0];
        }
        i += stride;
        if (i >= nlanes) break;
        r += dr; jw += dj;
        if (jw >= lw) { jw -= lw; ++r; }
    }
}

unsigned rows_blocks(int64_t items)
{
    int64_t blocks = (items + 255) / 256;
    if (blocks > (int64_t)device_cus() * 8) blocks = (int64_t)device_cus() * 8;
    return (unsigned)(blocks < 1 ? 1 : blocks);
}

// the rows a launch can have to cover: the total is known on the device only, the capacity bounds it
static int64_t rows_bound(const RowsParams &p) { return p.rows_cap < ((int64_t)1 << 40) ? p.rows_cap : ((int64_t)1 << 40); }

void launch_rows_count(const RowsParams &p, hipStream_t s) { hipLaunchKernelGGL(k_rows_count, dim3(rows_blocks(p.nseq)), dim3(256), 0, s, p); }
void launch_rows_map(const RowsParams &p, hipStream_t s) { hipLaunchKernelGGL(k_rows_map, dim3(rows_blocks(rows_bound(p))), dim3(256), 0, s, p); }

void launch_rows_fill(const RowsParams &p, hipStream_t s)
{
    const bool wide = p.spec.row_len % 4 == 0 && ((uintptr_t)p.rows & 15) == 0 && ((uintptr_t)p.mask & 3) == 0;
    const int64_t lanes = rows_bound(p) * (p.spec.row_len / (wide ? 4 : 1));
    if (wide) hipLaunchKernelGGL(k_rows_fill<4>, dim3(rows_blocks(lanes)), dim3(256), 0, s, p);
    else hipLaunchKernelGGL(k_rows_fill<1>, dim3(rows_blocks(lanes)), dim3(256), 0, s, p);
}

} // namespace bfa
