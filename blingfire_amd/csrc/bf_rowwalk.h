// bf_rowwalk.h -- the walk over rows that are already there, once for k_rows_span, k_rows_mlm, k_rows_mlm_cap and k_rows_denoise (device only;
// tests/hosttest/rowwalk_emu.h is the host emulation).
//
// The partition: G = span_group(row_len) lanes share a row -- a wave, or a power-of-two slice of one for rows of at most 32 cells: 64 / G rows per
// wave.  The row bound is min(*nrows, rows_cap), read on the device.  Round k of the grid gives a wave the 64 / G rows from wave_row + k * per_grid
// on; every wave of the grid makes the same number of rounds, and a row past the end is a group that is not `live`: it loads and stores nothing
// but takes part in every shuffle, ballot and vote, so no cross-lane operation is under divergent control flow.  A kernel that walks a row in
// chunks walks them in order, lane l at cell j0 + l (coalesced dword loads and stores), with loop bounds that depend on row_len alone.
#pragma once
#include "bf_kernels_common.h"

namespace bfa {

// The kernels write
//     const int64_t nrows = rows_bound(p.nrows, p.rows_cap);
//     const int lane = group_lane<G>();
//     for (int64_t step = rows_per_round<G>(B), r0 = wave_first_row<G>(B); r0 < nrows; r0 += step) {
//         const int64_t r = group_row<G>(r0);
//         const bool live = r < nrows;
// (functions of the lane and nothing kept in a struct: that is the form that compiles to the code of the loop written out in each kernel.)
// B = the lanes of a block: the constant every launch of the kernel uses, or blockDim.x where the launcher sizes the block (with a constant the
// divisions fold to shifts).
__device__ __forceinline__ int64_t rows_bound(const int64_t *nrows_dev, int64_t rows_cap)
{
    int64_t nrows = nrows_dev ? *nrows_dev : rows_cap;
    if (nrows > rows_cap) nrows = rows_cap;
    return nrows;
}
template <int G> __device__ __forceinline__ int group_lane() { return threadIdx.x & (G - 1); }                                  // the lane within its group
template <int G> __device__ __forceinline__ int64_t rows_per_round(unsigned block) { return (int64_t)gridDim.x * (block / G); } // rows per round of the grid
template <int G> __device__ __forceinline__ int64_t wave_first_row(unsigned block)                                             // the first row of this wave's round
{
    return ((int64_t)blockIdx.x * block + (threadIdx.x & ~63u)) / G;
}
template <int G> __device__ __forceinline__ int64_t group_row(int64_t r0) { return r0 + (threadIdx.x & 63) / G; }               // the row of this lane's group

// the lanes of this lane's group in a ballot: in place (to count them), and shifted down to bit 0 (to index by the lane within the group)
struct GroupBallot {
    int shift;                         // the group's first lane in the wave
    uint64_t group;                    // the group's lanes of a ballot
    __device__ __forceinline__ uint64_t in_place(bool pred) const { return __ballot(pred) & group; }
    __device__ __forceinline__ uint64_t operator()(bool pred) const { return (__ballot(pred) & group) >> shift; }
};
template <int G> __device__ __forceinline__ GroupBallot group_ballots()
{
    const int shift = (int)(threadIdx.x & 63u) & ~(G - 1);
    return GroupBallot{shift, (G == 64 ? ~(uint64_t)0 : (((uint64_t)1 << G) - 1)) << shift};
}

// ---- the whole-word head of a chunk (bf_mlm.h has the lane arithmetic).  h of cell j: the end and the "joins a unit" flag of cell j - 1 come one
// lane up (lane 0: the carry of the chunk before), the head is an inclusive max-scan of (continues ? -1 : j) in log2 G steps, lanes still at -1
// take the carried head, and the last lane's (end, joins, head) is the next chunk's carry.  Returns both: `h = m.h; carry = m.carry;`.  (The
// cell's values by reference and the carry by value: the forms in which the kernels keep the registers of the code written out in place.)
struct MlmHead { int h; MlmCarry carry; };
template <int G> __device__ __forceinline__ MlmHead mlm_chunk_head(const bool &eligible, const int32_t &S, const int32_t &E, int j, int lane, MlmCarry carry)
{
    const int joins = mlm_joins(eligible, S) ? 1 : 0;
    int32_t end_prev = __shfl_up(E, 1, G);
    int joins_prev = __shfl_up(joins, 1, G);
    if (lane == 0) { end_prev = carry.end; joins_prev = carry.joins; }
    int h = mlm_head_seed(mlm_continues(joins_prev != 0, end_prev, joins != 0, S), j);
#pragma unroll
    for (int d = 1; d < G; d <<= 1) h = mlm_head_step(h, __shfl_up(h, d, G), lane >= d);
    h = mlm_head_close(h, carry.head);
    return MlmHead{h, MlmCarry{__shfl(E, G - 1, G), __shfl(joins, G - 1, G), __shfl(h, G - 1, G)}};
}

// ---- the launch side: f(std::integral_constant<int, G>{}) for G = span_group(row_len); the grid of G lanes per row (the row count is on the
// device: the capacity bounds it, itself bounded so that the product cannot overflow)
template <class F> static void dispatch_span_group(int row_len, F &&f)
{
    switch (span_group(row_len)) {
    case 1: f(std::integral_constant<int, 1>{}); break;
    case 2: f(std::integral_constant<int, 2>{}); break;
    case 4: f(std::integral_constant<int, 4>{}); break;
    case 8: f(std::integral_constant<int, 8>{}); break;
    case 16: f(std::integral_constant<int, 16>{}); break;
    case 32: f(std::integral_constant<int, 32>{}); break;
    default: f(std::integral_constant<int, 64>{}); break;
    }
}

static inline int64_t rows_bounded(int64_t rows_cap) { return rows_cap < ((int64_t)1 << 40) ? rows_cap : ((int64_t)1 << 40); }
static inline unsigned rows_grid(int64_t rows_cap, int G) { return rows_blocks(rows_bounded(rows_cap) * G); }

} // namespace bfa
