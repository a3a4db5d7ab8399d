// bf_kernels_stream.hip -- ragged ids -> stream rows: the units laid end to end and cut into rows of exactly row_len cells, with next-token labels,
// a segment and a position plane (bf_stream.h has the lane code and what a cell is; include/blingfiretokdll_amd.h IdsToStreamRowsBatchDevice is
// the specification).
//
//  k_stream_widths  lane per sequence: a range outside its array or with decreasing offsets, and a sequence too long for an int32 width, is read
//                   as empty (status bit 3); the width of its unit.
//  (scan)           k_scan_* of bf_kernels_sp.hip over the widths -> W; T = W[nseq].
//  k_stream_seq     lane per sequence: seq_row / seq_col; the lane of index nseq writes {R, T} and reports rows beyond rows_cap (status bit 0).
//  k_stream_fill    the flat cell space min(R, rows_cap) x row_len IS the stream: a workgroup takes tiles of 256 x C consecutive cells (C = 4 with
//                   row_len % 4 == 0 and every taken plane 16-byte aligned: one 16-byte store per plane; else 1).  Per tile, three waves search
//                   the whole W together, a probe per lane and round with a ballot (at most six rounds): the unit of the tile's first cell, the unit of
//                   the cell behind its last one (a label reads one element past a lane's cells: the slice is staged one unit further, nothing is
//                   searched again), the first unit of the row the tile begins in.  The slice W[qa .. qe + 1] goes to LDS relative to the tile,
//                   with off[q] - W[q] - lead per unit, so an id cell is ids[t + delta].  A lane finds the unit of its first cell by a binary search
//                   of the LDS slice and carries it over its cells.  A slice of more than STREAM_STAGE_UNITS units (runs of units of width 0 are
//                   unbounded) is not staged: the lanes search global W between the tile's two bounds, through the same lane code.
//                   The lane whose first cell opens a row writes the row's first sequence and position.
// No lane walks a unit's cells or a run of empty units.  No workspace is sized by the row count: R is not bounded by nseq here.
#include "bf_kernels_common.h"

namespace bfa {

__global__ __launch_bounds__(256) void k_stream_widths(StreamParams p)
{
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < p.nseq; q += stride) {
        bool bad;
        p.widths[q] = stream_width(p.spec, p.id_off[q], p.id_off[q + 1], p.ids_len, &bad);
        if (bad) atomicOr(p.status, BF_STATUS_BAD_OFFSETS);
    }
}

__global__ __launch_bounds__(256) void k_stream_seq(StreamParams p)
{
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q <= p.nseq; q += stride) {
        const int64_t Wq = p.W[q];
        if (q == p.nseq) {                                  // Wq = T
            const int64_t R = stream_nrows(p.spec, Wq);
            p.nrows[0] = R; p.nrows[1] = Wq;
            if (R > p.rows_cap && (p.rows || p.seg || p.pos || p.labels || p.row_first_seq || p.row_first_pos)) atomicOr(p.status, 1);
            continue;
        }
        int32_t row, col;
        stream_seq_cell(p.spec, Wq, &row, &col);
        if (p.seq_row) p.seq_row[q] = row;
        if (p.seq_col) p.seq_col[q] = col;
    }
}

// the last q in [0, nseq) with W[q] <= t (t < T = W[nseq]), by the 64 lanes of the calling wave together; the answer is wave-uniform
__device__ __forceinline__ int64_t wave_find_unit(const int64_t *W, int64_t nseq, int64_t t)
{
    int64_t lo = 0, hi = nseq;
    const int lane = lane_id();
    while (hi - lo > 1) {
        const int64_t at = stream_probe(lo, hi, lane);
        const bool yes = at >= 0 && W[at] <= t;
        stream_narrow(&lo, &hi, __ballot(yes));
    }
    return lo;
}

// The six output pointers are needed at a tile's stores alone.  Kept in scalar registers across the cell code they push other uniform values of
// the kernel out (the wide form spilled 7 scalar registers into lanes of a vector register, 106 in use); so the store reads them from the
// kernel's own argument block again, tile by tile (92 in use, none spilled): the block's address goes through an empty asm, which keeps the
// compiler from hoisting those loads out of the loop.
typedef const __attribute__((address_space(4))) StreamParams *StreamArgs;
__device__ __forceinline__ StreamArgs stream_args()
{
    StreamArgs a = (StreamArgs)__builtin_amdgcn_kernarg_segment_ptr();       // (the kernel's one parameter lies at the block's start)
    asm volatile("" : "+s"(a));
    return a;
}

template <int C, class P>
__device__ __forceinline__ void stream_store(const P &p, int64_t at, int64_t r, int j, const StreamCell *c, int32_t first_seq, int32_t first_pos)
{
    if constexpr (C == 4) {
        if (p.rows) *(int4 *)(p.rows + at) = make_int4(c[0].id, c[1].id, c[2].id, c[3].id);
        if (p.seg) *(int4 *)(p.seg + at) = make_int4(c[0].seg, c[1].seg, c[2].seg, c[3].seg);
        if (p.pos) *(int4 *)(p.pos + at) = make_int4(c[0].pos, c[1].pos, c[2].pos, c[3].pos);
        if (p.labels) *(int4 *)(p.labels + at) = make_int4(c[0].label, c[1].label, c[2].label, c[3].label);
    } else {
        if (p.rows) p.rows[at] = c[0].id;
        if (p.seg) p.seg[at] = c[0].seg;
        if (p.pos) p.pos[at] = c[0].pos;
        if (p.labels) p.labels[at] = c[0].label;
    }
    if (j == 0) {
        if (p.row_first_seq) p.row_first_seq[r] = first_seq;
        if (p.row_first_pos) p.row_first_pos[r] = first_pos;
    }
}

// C cells per lane: 4 = the aligned form, 1 = any row_len and any base
template <int C>
__global__ __launch_bounds__(256) void k_stream_fill(StreamParams p)
{
    constexpr int TC = STREAM_TILE_LANES * C;
    __shared__ int64_t s_delta[STREAM_STAGE_UNITS];
    __shared__ int32_t s_wrel[STREAM_STAGE_UNITS + 1];
    __shared__ int64_t s_found[3];
    const int L = p.spec.row_len;
    const int64_t T = p.W[p.nseq], R = stream_nrows(p.spec, T);
    const int64_t cells = (R < p.rows_cap ? R : p.rows_cap) * L;
    const bool want_label = p.labels != nullptr;
    const int wave = wave_in_block();
    // the lane's (row, place in the row) moves by a fixed step from one tile of the workgroup to its next: one division per lane, none per tile
    const int64_t step = (int64_t)gridDim.x * TC;
    int64_t t0 = (int64_t)blockIdx.x * TC;
    if (t0 >= cells) return;
    int64_t t = t0 + (int64_t)threadIdx.x * C;
    int64_t r = t / L;
    int j = (int)(t - r * L);
    const int64_t dr = step / L;
    const int dj = (int)(step - dr * L);
    for (;;) {
        StreamCell c[C];
        int32_t first_seq = 0, first_pos = 0;
        if (t0 >= T) {                                       // (the padding behind the stream: every lane of the tile)
            if (t < cells) stream_cells<C>(p.spec, StreamGlobal{}, p.ids, T, t0, 0, t, j, want_label, c, &first_seq, &first_pos);
        } else {
            if (wave < 3) {
                // wave 0: the first unit of the row the tile begins in (its first lane holds the tile's first cell: t = t0, at place j of its row);
                // wave 1: the unit of the tile's first cell; wave 2: the unit of the cell behind its last one
                const int64_t last = t0 + TC < T - 1 ? t0 + TC : T - 1;
                const int64_t target = wave == 0 ? t0 - __builtin_amdgcn_readfirstlane(j) : wave == 1 ? t0 : last;
                const int64_t q = wave_find_unit(p.W, p.nseq, target);
                if (lane_id() == 0) s_found[wave] = q;
            }
            __syncthreads();
            const int64_t f0 = s_found[0], qa = s_found[1], qe = s_found[2];
            const int64_t n = qe - qa + 1;
            if (n <= STREAM_STAGE_UNITS) {
                for (int i = (int)threadIdx.x; i <= (int)n; i += 256) {
                    const int64_t Wq = p.W[qa + i];
                    s_wrel[i] = stream_wrel(Wq, t0);
                    if (i < (int)n) s_delta[i] = stream_delta(p.id_off[qa + i], Wq, p.spec.lead);
                }
                __syncthreads();
                if (t < cells) stream_cells<C>(p.spec, StreamStaged{s_wrel, s_delta, t0, qa, (int)n}, p.ids, T, t0, f0, t, j, want_label, c, &first_seq, &first_pos);
            } else {
                if (t < cells) stream_cells<C>(p.spec, StreamGlobal{p.W, p.id_off, qa, qe, p.spec.lead}, p.ids, T, t0, f0, t, j, want_label, c, &first_seq, &first_pos);
            }
        }
        if (t < cells) stream_store<C>(*stream_args(), t, r, j, c, first_seq, first_pos);
        t0 += step;
        if (t0 >= cells) break;
        t += step; r += dr; j += dj;
        if (j >= L) { j -= L; ++r; }
        __syncthreads();                                      // the staged slice and the three answers are read; the next tile may overwrite them
    }
}

void launch_stream_widths(const StreamParams &p, hipStream_t s) { hipLaunchKernelGGL(k_stream_widths, dim3(rows_blocks(p.nseq)), dim3(256), 0, s, p); }
void launch_stream_seq(const StreamParams &p, hipStream_t s) { hipLaunchKernelGGL(k_stream_seq, dim3(rows_blocks(p.nseq + 1)), dim3(256), 0, s, p); }

// rows_bound = the host-known bound of R (stream_rows_bound): R is known on the device only
void launch_stream_fill(const StreamParams &p, int64_t rows_bound, hipStream_t s)
{
    const int L = p.spec.row_len;
    const bool wide = L % 4 == 0 && (((uintptr_t)p.rows | (uintptr_t)p.seg | (uintptr_t)p.pos | (uintptr_t)p.labels) & 15) == 0;
    const int64_t rows = p.rows_cap < rows_bound ? p.rows_cap : rows_bound;
    const int tc = STREAM_TILE_LANES * (wide ? STREAM_WIDE_CELLS : 1);
    const int64_t tiles = (rows * L + tc - 1) / tc;
    if (tiles <= 0) return;
    if (wide) hipLaunchKernelGGL(k_stream_fill<STREAM_WIDE_CELLS>, dim3(rows_blocks(tiles * 256)), dim3(256), 0, s, p);
    else hipLaunchKernelGGL(k_stream_fill<1>, dim3(rows_blocks(tiles * 256)), dim3(256), 0, s, p);
}

} // namespace bfa
