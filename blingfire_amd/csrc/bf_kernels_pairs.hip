// bf_kernels_pairs.hip -- pairs of ragged id sequences -> fixed-shape model inputs with type ids (bf_pairs.h has the cell logic and what a row is).
//
//  k_pairs_count  lane per pair: a range outside [0, len] or with decreasing offsets makes that side empty (status bit 3); the pair's own
//                 geometry from (na, nb), its windows -> counts.
//  (scan)         k_scan_* of bf_kernels_sp.hip over the counts -> row offsets; the row total stays on the device.
//  k_pairs_map    lane per row below min(total, rows_cap): its pair by binary search of the row offsets, the index within B of its first
//                 B id with the step of that pair (saturating at INT32_MAX); rows beyond rows_cap, and a saturated index, are reported
//                 (status bit 0).  Where one row per pair is certain (mode 1, max_rows_per_pair 1) row r is pair r: no search, here or below.
//  k_pairs_fill   lane per four cells (row_len % 4 == 0 and the three outputs aligned: one 16-byte store of ids, 4-byte stores of mask
//                 and type) or per cell, over the flat cell space min(total, rows_cap) x row_len.  A lane takes its pair's geometry from
//                 the four offsets again.  Ids are read with plain dword loads: a sequence starts anywhere.
// No lane walks a pair's windows or a row's cells.
#include "bf_kernels_common.h"
#include "bf_pairs.h"

namespace bfa {

// one side of pair q as the kernels see it: its ids (n of them: 0 for a bad range)
struct PairSide { const int32_t *seq; int64_t n; bool bad; };

__device__ __forceinline__ PairSide pair_side(const int32_t *ids, int64_t len, const int64_t *off, int64_t q)
{
    PairSide d;
    const int64_t b = off[q];
    d.n = rows_seq_len(b, off[q + 1], len, &d.bad);
    d.seq = ids + (d.bad ? 0 : b);
    return d;
}

__global__ __launch_bounds__(256) void k_pairs_count(PairsParams p)
{
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < p.nseq; q += stride) {
        const PairSide a = pair_side(p.ids_a, p.len_a, p.off_a, q), b = pair_side(p.ids_b, p.len_b, p.off_b, q);
        bool sat;
        p.counts[q] = pairs_count(p.spec, pairs_geom(p.spec, a.n, b.n), b.n, &sat);
        if (a.bad || b.bad) atomicOr(p.status, BF_STATUS_BAD_OFFSETS);
        if (sat) atomicOr(p.status, 1);
    }
}

// the index within B of the first B id of row r of pair q
__device__ __forceinline__ int64_t pair_first_b(const PairsParams &p, int64_t q, int64_t r, const PairGeom &g)
{
    return p.spec.mode == 0 ? (r - p.row_off[q]) * g.step : 0;
}

__global__ __launch_bounds__(256) void k_pairs_map(PairsParams p)
{
    const int64_t total = p.row_off[p.nseq], nrows = total < p.rows_cap ? total : p.rows_cap;
    const int64_t stride = (int64_t)gridDim.x * 256, r0 = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r0 == 0 && total > p.rows_cap) atomicOr(p.status, 1);
    for (int64_t r = r0; r < nrows; r += stride) {
        const int64_t q = pairs_one_row(p.spec) ? r : rows_find_seq(p.row_off, p.nseq, r);
        if (r < p.seq_rows) p.row_seq[r] = (int32_t)q;
        const PairSide a = pair_side(p.ids_a, p.len_a, p.off_a, q), b = pair_side(p.ids_b, p.len_b, p.off_b, q);
        bool sat;
        const int32_t first = rows_first_i32(pair_first_b(p, q, r, pairs_geom(p.spec, a.n, b.n)), &sat);
        if (r < p.first_rows) p.row_first[r] = first;
        if (sat) atomicOr(p.status, 1);
    }
}

// W cells per lane: 4 = the aligned form, 1 = any row_len and any base
template <int W>
__global__ __launch_bounds__(256) void k_pairs_fill(PairsParams p)
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
        const bool one = pairs_one_row(p.spec);
        const int64_t q = one ? r : r < p.seq_rows ? (int64_t)p.row_seq[r] : rows_find_seq(p.row_off, p.nseq, r);
        const PairSide a = pair_side(p.ids_a, p.len_a, p.off_a, q), b = pair_side(p.ids_b, p.len_b, p.off_b, q);
        const PairGeom g = pairs_geom(p.spec, a.n, b.n);
        int64_t first = one ? 0 : r < p.first_rows ? (int64_t)p.row_first[r] : 0x7fffffff;
        if (first == 0x7fffffff) first = pair_first_b(p, q, r, g);                // not held, or saturated: from the offsets
        const PairRow w = pairs_row(p.spec, g, first, b.n);
        int32_t v[W]; uint8_t m[W], t[W];
#pragma unroll
        for (int k = 0; k < W; ++k) v[k] = pairs_cell_value(p.spec, pairs_cell(w, jw * W + k), a.seq, b.seq, &m[k], &t[k]);
        const int64_t at = r * p.spec.row_len + (int64_t)jw * W;
        if constexpr (W == 4) {
            if (p.rows) *(int4 *)(p.rows + at) = make_int4(v[0], v[1], v[2], v[3]);
            if (p.mask) *(uint32_t *)(p.mask + at) = (uint32_t)m[0] | ((uint32_t)m[1] << 8) | ((uint32_t)m[2] << 16) | ((uint32_t)m[3] << 24);
            if (p.type) *(uint32_t *)(p.type + at) = (uint32_t)t[0] | ((uint32_t)t[1] << 8) | ((uint32_t)t[2] << 16) | ((uint32_t)t[3] << 24);
        } else {
            if (p.rows) p.rows[at] = v[0];
            if (p.mask) p.mask[at] = m[0];
            if (p.type) p.type[at] = t[0];
        }
        i += stride;
        if (i >= nlanes) break;
        r += dr; jw += dj;
        if (jw >= lw) { jw -= lw; ++r; }
    }
}

// the rows a launch can have to cover: the total is known on the device only, the capacity bounds it
static int64_t pairs_bound(const PairsParams &p) { return p.rows_cap < ((int64_t)1 << 40) ? p.rows_cap : ((int64_t)1 << 40); }

void launch_pairs_count(const PairsParams &p, hipStream_t s) { hipLaunchKernelGGL(k_pairs_count, dim3(rows_blocks(p.nseq)), dim3(256), 0, s, p); }
void launch_pairs_map(const PairsParams &p, hipStream_t s) { hipLaunchKernelGGL(k_pairs_map, dim3(rows_blocks(pairs_bound(p))), dim3(256), 0, s, p); }

void launch_pairs_fill(const PairsParams &p, hipStream_t s)
{
    const bool wide = p.spec.row_len % 4 == 0 && ((uintptr_t)p.rows & 15) == 0 && ((uintptr_t)p.mask & 3) == 0 && ((uintptr_t)p.type & 3) == 0;
    const int64_t lanes = pairs_bound(p) * (p.spec.row_len / (wide ? 4 : 1));
    if (wide) hipLaunchKernelGGL(k_pairs_fill<4>, dim3(rows_blocks(lanes)), dim3(256), 0, s, p);
    else hipLaunchKernelGGL(k_pairs_fill<1>, dim3(rows_blocks(lanes)), dim3(256), 0, s, p);
}

} // namespace bfa
