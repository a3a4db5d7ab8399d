// bf_rowstage_body.h -- the row stage: items of a source S -> fixed-shape model inputs.  Included by bf_kernels_rows.hip (S = RowsSource, bf_rows.h:
// ragged ids) and bf_kernels_pairs.hip (S = PairsSource, bf_pairs.h: pairs of them), which instantiate the launchers at the end for their source.
// What a source supplies is listed at RowsSource; everything a source does not decide is here, once.
//
//  k_rowstage_count  lane per item: a range outside its array or with decreasing offsets is read as empty (status bit 3); its rows -> counts.
//  (scan)            k_scan_* of bf_kernels_sp.hip over the counts -> row offsets; the row total stays on the device.
//  k_rowstage_map    lane per row below min(total, rows_cap): its item by binary search of the row offsets (none where one row per item is
//                    certain: row r is item r, here and below), the index of its first id (saturating at INT32_MAX); rows beyond rows_cap,
//                    and a saturated index, are reported (status bit 0).
//  k_rowstage_fill   lane per four cells (row_len % 4 == 0 and every output aligned: one 16-byte store of ids, one 4-byte store per byte
//                    plane) or per cell, over the flat cell space min(total, rows_cap) x row_len.  A lane loads its item again.  Ids are read
//                    with plain dword loads: a sequence starts anywhere.
//  k_rowstage_planes (the ...Planes calls only, behind the kernels above) the fill's stepping over the same cell space; a lane asks the source where
//                    each of its cells reads (S::where) and gathers that element of every companion array, or takes the plane's fill.
// No lane walks an item's windows or a row's cells: one sequence of 10^5 windows is 10^5 rows like any others.
#pragma once
#include "bf_kernels_common.h"

namespace bfa {

template <class S>
__global__ __launch_bounds__(256) void k_rowstage_count(RowStageParams<S> p)
{
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < p.nseq; q += stride) {
        const typename S::Item it = p.src.load(q);
        bool sat;
        p.counts[q] = p.src.count(it, &sat);
        if (it.bad) atomicOr(p.status, BF_STATUS_BAD_OFFSETS);
        if (sat) atomicOr(p.status, 1);
    }
}

template <class S>
__global__ __launch_bounds__(256) void k_rowstage_map(RowStageParams<S> p)
{
    const int64_t total = p.row_off[p.nseq], nrows = total < p.rows_cap ? total : p.rows_cap;
    const int64_t stride = (int64_t)gridDim.x * 256, r0 = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r0 == 0 && total > p.rows_cap) atomicOr(p.status, 1);
    for (int64_t r = r0; r < nrows; r += stride) {
        const int64_t q = p.src.one_row() ? r : rows_find_seq(p.row_off, p.nseq, r);
        if (r < p.seq_rows) p.row_seq[r] = (int32_t)q;
        bool sat;
        const int32_t first = rows_first_i32(p.src.first(p.src.load(q), r - p.row_off[q]), &sat);
        if (r < p.first_rows) p.row_first[r] = first;
        if (sat) atomicOr(p.status, 1);
    }
}

__device__ __forceinline__ uint32_t rowstage_pack4(const uint8_t *b) { return (uint32_t)b[0] | ((uint32_t)b[1] << 8) | ((uint32_t)b[2] << 16) | ((uint32_t)b[3] << 24); }

// W cells per lane: 4 = the aligned form, 1 = any row_len and any base
template <class S, int W>
__global__ __launch_bounds__(256) void k_rowstage_fill(RowStageParams<S> p)
{
    const int64_t total = p.row_off[p.nseq], nrows = total < p.rows_cap ? total : p.rows_cap;
    const int row_len = p.src.spec.row_len, lw = row_len / W;          // lanes per row
    const int64_t nlanes = nrows * lw, stride = (int64_t)gridDim.x * 256;
    int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nlanes) return;
    // the lane's (row, place in the row) moves by a fixed step from one round to the next: one division per lane, none per round
    int64_t r = i / lw;
    int jw = (int)(i - r * lw);
    const int64_t dr = stride / lw;
    const int dj = (int)(stride - dr * lw);
    for (;;) {
        const bool one = p.src.one_row();
        const int64_t q = one ? r : r < p.seq_rows ? (int64_t)p.row_seq[r] : rows_find_seq(p.row_off, p.nseq, r);
        const typename S::Item it = p.src.load(q);
        int64_t first = one ? 0 : r < p.first_rows ? (int64_t)p.row_first[r] : 0x7fffffff;
        if (first == 0x7fffffff) first = p.src.first(it, r - p.row_off[q]);      // not held, or saturated: from the offsets
        const typename S::Row w = p.src.row(it, first);
        int32_t v[W]; uint8_t m[W], t[W];
#pragma unroll
        for (int k = 0; k < W; ++k) v[k] = p.src.cell(it, w, jw * W + k, &m[k], &t[k]);
        const int64_t at = r * row_len + (int64_t)jw * W;
        if constexpr (W == 4) {
            if (p.rows) *(int4 *)(p.rows + at) = make_int4(v[0], v[1], v[2], v[3]);
            if (p.mask) *(uint32_t *)(p.mask + at) = rowstage_pack4(m);
            if constexpr (S::HAS_TYPE) if (p.type) *(uint32_t *)(p.type + at) = rowstage_pack4(t);
        } else {
            if (p.rows) p.rows[at] = v[0];
            if (p.mask) p.mask[at] = m[0];
            if constexpr (S::HAS_TYPE) if (p.type) p.type[at] = t[0];
        }
        i += stride;
        if (i >= nlanes) break;
        r += dr; jw += dj;
        if (jw >= lw) { jw -= lw; ++r; }
    }
}

// W cells per lane, as in the fill: 4 = row_len % 4 == 0 and every taken plane aligned to 16 bytes (one 16-byte store per plane), 1 = anything.
// The sources are read with plain dword loads: a sequence starts anywhere.
template <class S, int W>
__global__ __launch_bounds__(256) void k_rowstage_planes(RowPlanesParams<S> pp)
{
    const RowStageParams<S> &p = pp.st;
    const int64_t total = p.row_off[p.nseq], nrows = total < p.rows_cap ? total : p.rows_cap;
    const int row_len = p.src.spec.row_len, lw = row_len / W;          // lanes per row
    const int64_t nlanes = nrows * lw, stride = (int64_t)gridDim.x * 256;
    int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nlanes) return;
    int64_t r = i / lw;                                                // (one division per lane, none per round: k_rowstage_fill)
    int jw = (int)(i - r * lw);
    const int64_t dr = stride / lw;
    const int dj = (int)(stride - dr * lw);
    for (;;) {
        const bool one = p.src.one_row();
        const int64_t q = one ? r : r < p.seq_rows ? (int64_t)p.row_seq[r] : rows_find_seq(p.row_off, p.nseq, r);
        const typename S::Item it = p.src.load(q);
        int64_t first = one ? 0 : r < p.first_rows ? (int64_t)p.row_first[r] : 0x7fffffff;
        if (first == 0x7fffffff) first = p.src.first(it, r - p.row_off[q]);      // not held, or saturated: from the offsets
        const typename S::Row w = p.src.row(it, first);
        CellWhere c[W];
#pragma unroll
        for (int k = 0; k < W; ++k) c[k] = p.src.where(it, w, jw * W + k);
        const int64_t at = r * row_len + (int64_t)jw * W;
#pragma unroll
        for (int k = 0; k < ROWS_MAX_PLANES; ++k) {
            if (k >= pp.nplanes || !pp.out[k]) continue;
            int32_t v[W];
#pragma unroll
            for (int x = 0; x < W; ++x) {
                const int32_t *from = c[x].side < 0 ? nullptr : c[x].side == CELL_SIDE_B ? pp.src[CELL_SIDE_B][k] : pp.src[CELL_SIDE_A][k];      // (a selection: the side is the lane's)
                v[x] = from ? from[c[x].at] : pp.fill[k];
            }
            if constexpr (W == 4) *(int4 *)(pp.out[k] + at) = make_int4(v[0], v[1], v[2], v[3]);
            else pp.out[k][at] = v[0];
        }
        i += stride;
        if (i >= nlanes) break;
        r += dr; jw += dj;
        if (jw >= lw) { jw -= lw; ++r; }
    }
}

// the rows a launch can have to cover: the total is known on the device only, the capacity bounds it
template <class S>
static int64_t rows_bound(const RowStageParams<S> &p) { return p.rows_cap < ((int64_t)1 << 40) ? p.rows_cap : ((int64_t)1 << 40); }

template <class S>
void launch_rowstage_count(const RowStageParams<S> &p, hipStream_t s) { hipLaunchKernelGGL(k_rowstage_count<S>, dim3(rows_blocks(p.nseq)), dim3(256), 0, s, p); }
template <class S>
void launch_rowstage_map(const RowStageParams<S> &p, hipStream_t s) { hipLaunchKernelGGL(k_rowstage_map<S>, dim3(rows_blocks(rows_bound(p))), dim3(256), 0, s, p); }

template <class S>
void launch_rowstage_fill(const RowStageParams<S> &p, hipStream_t s)
{
    const int row_len = p.src.spec.row_len;
    const bool wide = row_len % 4 == 0 && ((uintptr_t)p.rows & 15) == 0 && ((uintptr_t)p.mask & 3) == 0 && ((uintptr_t)p.type & 3) == 0;
    const int64_t lanes = rows_bound(p) * (row_len / (wide ? 4 : 1));
    if (wide) hipLaunchKernelGGL((k_rowstage_fill<S, 4>), dim3(rows_blocks(lanes)), dim3(256), 0, s, p);
    else hipLaunchKernelGGL((k_rowstage_fill<S, 1>), dim3(rows_blocks(lanes)), dim3(256), 0, s, p);
}

template <class S>
void launch_rowstage_planes(const RowPlanesParams<S> &pp, hipStream_t s)
{
    const int row_len = pp.st.src.spec.row_len;
    bool wide = row_len % 4 == 0;
    for (int k = 0; k < pp.nplanes; ++k) wide = wide && ((uintptr_t)pp.out[k] & 15) == 0;
    const int64_t lanes = rows_bound(pp.st) * (row_len / (wide ? 4 : 1));
    if (wide) hipLaunchKernelGGL((k_rowstage_planes<S, 4>), dim3(rows_blocks(lanes)), dim3(256), 0, s, pp);
    else hipLaunchKernelGGL((k_rowstage_planes<S, 1>), dim3(rows_blocks(lanes)), dim3(256), 0, s, pp);
}

} // namespace bfa
