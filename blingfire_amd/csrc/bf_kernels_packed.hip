// bf_kernels_packed.hip -- ragged ids -> packed rows: several sequences per row, a segment plane and a position plane (bf_packed.h has the
// lane code and what a row is; include/blingfiretokdll_amd.h IdsToPackedRowsBatchDevice is the specification).
//
//  k_packed_widths  lane per sequence: a range outside its array or with decreasing offsets is read as empty (status bit 3); the width of its unit.
//  (scan)           k_scan_* of bf_kernels_sp.hip over the widths -> W.
//  k_packed_next    lane per sequence: next(s) by a galloping search of W, next(nseq) = nseq; mark = {0}.
//  k_packed_double  one launch per round, lane per sequence: a marked s marks its jump, every jump is squared into the other buffer.  After
//                   packed_rounds(nseq) rounds exactly the sequences a row starts at are marked.  The host counts the rounds from nseq alone.
//  (scan)           over the marks -> the row of every sequence; the total is R.
//  k_packed_rows    lane per sequence: a marked sequence writes itself to f[its row] (and to the caller's row_first below rows_cap); seq_row;
//                   the lane of index nseq writes f[R] = nseq, R, and reports rows beyond rows_cap (status bit 0).
//  k_packed_cols    lane per sequence: seq_col = W[q] - W[f[row]].
//  k_packed_fill    lane per four cells (row_len % 4 == 0 and every plane 16-byte aligned: one 16-byte store per plane) or per cell, over the flat
//                   cell space min(R, rows_cap) x row_len, stepping like k_rowstage_fill.  A lane finds its unit by a binary search of the row's own
//                   slice W[f[r] .. f[r+1]]: the lanes of a row read the same few cache lines, usually 4 .. 20 entries, so the slice is not staged in
//                   LDS (a row maps to no fixed group of lanes: row_len is any number from 1 to 2^20).
//  k_packed_planes  (IdsToPackedRowsPlanesBatch only, behind the kernels above) the fill's cell space, stepping and two forms; a lane finds its unit
//                   by the same search and gathers, for each of its cells, the element of every companion array that the cell's id has.
// No lane walks the chain of rows, a row's units or a unit's cells: 10^5 empty sequences in one row cost a search of 17 steps.
#include "bf_kernels_common.h"

namespace bfa {

__global__ __launch_bounds__(256) void k_packed_widths(PackedParams p)
{
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < p.nseq; q += stride) {
        bool bad;
        const int64_t n = rows_seq_len(p.id_off[q], p.id_off[q + 1], p.ids_len, &bad);
        p.widths[q] = packed_width(p.spec, n);
        if (bad) atomicOr(p.status, BF_STATUS_BAD_OFFSETS);
    }
}

__global__ __launch_bounds__(256) void k_packed_next(PackedParams p)
{
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x; s <= p.nseq; s += stride) {
        p.jmp[0][s] = s < p.nseq ? packed_next(p.W, p.nseq, s, p.spec.row_len) : (int32_t)p.nseq;
        p.mark[s] = s == 0 ? 1 : 0;
    }
}

__global__ __launch_bounds__(256) void k_packed_double(const int32_t *jin, int32_t *jout, int32_t *mark, int64_t nseq)
{
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x; s <= nseq; s += stride) packed_double(jin, jout, mark, s);
}

__global__ __launch_bounds__(256) void k_packed_rows(PackedParams p)
{
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q <= p.nseq; q += stride) {
        const int64_t r = p.mark_off[q];
        if (q == p.nseq) {                                  // r = R
            p.f[r] = (int32_t)q;
            if (p.row_first && r <= p.rows_cap) p.row_first[r] = (int32_t)q;
            p.nrows[0] = r;
            if (r > p.rows_cap && (p.rows || p.seg || p.pos || p.row_first)) atomicOr(p.status, 1);
            continue;
        }
        const int m = p.mark[q];
        if (m) {
            p.f[r] = (int32_t)q;
            if (p.row_first && r <= p.rows_cap) p.row_first[r] = (int32_t)q;
        }
        if (p.seq_row) p.seq_row[q] = (int32_t)(r + m - 1);
    }
}

__global__ __launch_bounds__(256) void k_packed_cols(PackedParams p)
{
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < p.nseq; q += stride)
        p.seq_col[q] = (int32_t)(p.W[q] - p.W[p.f[p.mark_off[q] + p.mark[q] - 1]]);
}

// C cells per lane: 4 = the aligned form, 1 = any row_len and any base
template <int C>
__global__ __launch_bounds__(256) void k_packed_fill(PackedParams p)
{
    const int64_t total = p.mark_off[p.nseq], nrows = total < p.rows_cap ? total : p.rows_cap;
    const int row_len = p.spec.row_len, lw = row_len / C;              // lanes per row
    const int64_t nlanes = nrows * lw, stride = (int64_t)gridDim.x * 256;
    int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nlanes) return;
    // the lane's (row, place in the row) moves by a fixed step from one round to the next: one division per lane, none per round
    int64_t r = i / lw;
    int jw = (int)(i - r * lw);
    const int64_t dr = stride / lw;
    const int dj = (int)(stride - dr * lw);
    for (;;) {
        const int64_t s = p.f[r], e = p.f[r + 1];
        int64_t q = s;
        PackedCell c[C];
#pragma unroll
        for (int k = 0; k < C; ++k) c[k] = packed_cell(p.spec, p.W, s, e, jw * C + k, p.ids, p.id_off, &q);
        const int64_t at = r * row_len + (int64_t)jw * C;
        if constexpr (C == 4) {
            if (p.rows) *(int4 *)(p.rows + at) = make_int4(c[0].id, c[1].id, c[2].id, c[3].id);
            if (p.seg) *(int4 *)(p.seg + at) = make_int4(c[0].seg, c[1].seg, c[2].seg, c[3].seg);
            if (p.pos) *(int4 *)(p.pos + at) = make_int4(c[0].pos, c[1].pos, c[2].pos, c[3].pos);
        } else {
            if (p.rows) p.rows[at] = c[0].id;
            if (p.seg) p.seg[at] = c[0].seg;
            if (p.pos) p.pos[at] = c[0].pos;
        }
        i += stride;
        if (i >= nlanes) break;
        r += dr; jw += dj;
        if (jw >= lw) { jw -= lw; ++r; }
    }
}

// The companion planes, behind the fill: the fill's cell space and stepping, C cells per lane in the same two forms.  A lane asks packed_where --
// the fill's steps with the fetch left out (bf_packed.h) -- which element each of its cells holds and gathers that element of every source, or takes the plane's
// fill.  The sources are read with plain dword loads: a sequence starts anywhere.  No LDS, no atomics but the one status report: k_packed_rows
// reports rows dropped from the base outputs, lane 0 here those dropped from a plane (the call may take planes alone).
template <int C>
__global__ __launch_bounds__(256) void k_packed_planes(PackedPlanesParams pp)
{
    const PackedParams &p = pp.pk;
    const int64_t total = p.mark_off[p.nseq], nrows = total < p.rows_cap ? total : p.rows_cap;
    const int row_len = p.spec.row_len, lw = row_len / C;              // lanes per row
    const int64_t nlanes = nrows * lw, stride = (int64_t)gridDim.x * 256;
    int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i == 0 && total > p.rows_cap) atomicOr(p.status, 1);
    if (i >= nlanes) return;
    int64_t r = i / lw;                                                // (one division per lane, none per round: k_packed_fill)
    int jw = (int)(i - r * lw);
    const int64_t dr = stride / lw;
    const int dj = (int)(stride - dr * lw);
    for (;;) {
        const int64_t s = p.f[r], e = p.f[r + 1];
        int64_t q = s;
        int64_t from[C];
#pragma unroll
        for (int k = 0; k < C; ++k) from[k] = packed_where(p.spec, p.W, s, e, jw * C + k, p.id_off, &q);
        const int64_t at = r * row_len + (int64_t)jw * C;
#pragma unroll
        for (int k = 0; k < ROWS_MAX_PLANES; ++k) {
            if (k >= pp.nplanes || !pp.out[k]) continue;
            int32_t v[C];
#pragma unroll
            for (int x = 0; x < C; ++x) v[x] = from[x] != PACKED_NONE ? pp.src[k][from[x]] : pp.fill[k];
            if constexpr (C == 4) *(int4 *)(pp.out[k] + at) = make_int4(v[0], v[1], v[2], v[3]);
            else pp.out[k][at] = v[0];
        }
        i += stride;
        if (i >= nlanes) break;
        r += dr; jw += dj;
        if (jw >= lw) { jw -= lw; ++r; }
    }
}

void launch_packed_widths(const PackedParams &p, hipStream_t s) { hipLaunchKernelGGL(k_packed_widths, dim3(rows_blocks(p.nseq)), dim3(256), 0, s, p); }
void launch_packed_next(const PackedParams &p, hipStream_t s) { hipLaunchKernelGGL(k_packed_next, dim3(rows_blocks(p.nseq + 1)), dim3(256), 0, s, p); }
void launch_packed_double(const PackedParams &p, int round, hipStream_t s)
{
    hipLaunchKernelGGL(k_packed_double, dim3(rows_blocks(p.nseq + 1)), dim3(256), 0, s, (const int32_t *)p.jmp[round & 1], p.jmp[(round & 1) ^ 1], p.mark, p.nseq);
}
void launch_packed_rows(const PackedParams &p, hipStream_t s) { hipLaunchKernelGGL(k_packed_rows, dim3(rows_blocks(p.nseq + 1)), dim3(256), 0, s, p); }
void launch_packed_cols(const PackedParams &p, hipStream_t s) { hipLaunchKernelGGL(k_packed_cols, dim3(rows_blocks(p.nseq)), dim3(256), 0, s, p); }

void launch_packed_fill(const PackedParams &p, hipStream_t s)
{
    const int row_len = p.spec.row_len;
    const bool wide = row_len % 4 == 0 && (((uintptr_t)p.rows | (uintptr_t)p.seg | (uintptr_t)p.pos) & 15) == 0;
    const int64_t rows = p.rows_cap < p.nseq ? p.rows_cap : p.nseq;      // R is known on the device only; it is at most nseq
    const int64_t lanes = rows * (row_len / (wide ? 4 : 1));
    if (wide) hipLaunchKernelGGL(k_packed_fill<4>, dim3(rows_blocks(lanes)), dim3(256), 0, s, p);
    else hipLaunchKernelGGL(k_packed_fill<1>, dim3(rows_blocks(lanes)), dim3(256), 0, s, p);
}

// (with rows_cap = 0 one block: lane 0 still reports the rows dropped)
void launch_packed_planes(const PackedPlanesParams &pp, hipStream_t s)
{
    const PackedParams &p = pp.pk;
    const int row_len = p.spec.row_len;
    bool wide = row_len % 4 == 0;
    for (int k = 0; k < pp.nplanes; ++k) wide = wide && ((uintptr_t)pp.out[k] & 15) == 0;
    const int64_t rows = p.rows_cap < p.nseq ? p.rows_cap : p.nseq;      // (R is at most nseq: launch_packed_fill)
    const int64_t lanes = rows * (row_len / (wide ? 4 : 1));
    if (wide) hipLaunchKernelGGL(k_packed_planes<4>, dim3(rows_blocks(lanes)), dim3(256), 0, s, pp);
    else hipLaunchKernelGGL(k_packed_planes<1>, dim3(rows_blocks(lanes)), dim3(256), 0, s, pp);
}

} // namespace bfa
