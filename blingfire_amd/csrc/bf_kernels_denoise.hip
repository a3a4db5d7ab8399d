// bf_kernels_denoise.hip -- rows that are already there -> the encoder row and the decoder row of span corruption (bf_denoise.h has the lane code:
// the reach, the segmented scan, the run index and its cap, the running counts, the two positions; include/blingfiretokdll_amd.h
// RowsDenoiseBatchDevice is the specification).
//
//  k_rows_denoise<G>  bf_rowwalk.h's partition (G lanes share a row, every wave the same rounds and, inside a round, the same chunks: no cross-lane
//                     operation is divergent).  A row is walked ONCE, in chunks of G cells in order, lane l takes cell j0 + l.  Per chunk:
//     loads           the cell's id, mask byte and segment (coalesced); one Philox evaluation where the cell is eligible -> its reach.
//     scan            the segmented inclusive max-scan of (ineligible, reach) in log2 G steps of one shuffle (the pair travels as one word), closed
//                     with the carried reach.
//     neighbour       raw noise of the cell one lane up (lane 0: the carry) -> the run begins.
//     ballots         three, masked to the group's lanes: run begins (-> the run index by popcount, -> the cap), noise cells, kept cells; the
//                     capped begins are the begins that are still noise.  Popcounts below the lane plus the carry are the running counts.
//     stores          a kept cell to the encoder row, a begin's sentinel to both rows, a noise cell to the decoder row, each with its source
//                     cell (or -1): compacted in cell order, so neighbouring lanes write neighbouring or equal-distance addresses.
//                     After the last chunk the group fills the two tails, and lane 0 writes the eos, the three counts and, for a row that
//                     lost a cell of an output the caller takes, bit 0 of the status word (the kernel's only atomic).
// One pass, no LDS, no scratch.  An output position at or past enc_len / dec_len is not stored; positions are never negative, and rows at or
// past min(rows_cap, *nrows) are not touched: every store lies inside [0, rows_cap * len) of its plane.  The outputs must not overlap the inputs:
// the compacted rows are written in front of cells that lanes of a later chunk still read.
#include "bf_rowwalk.h"

namespace bfa {

template <int G>
__global__ __launch_bounds__(256) void k_rows_denoise(RowsDenoiseParams p)
{
    const int64_t nrows = rows_bound(p.nrows, p.rows_cap);
    const int lane = group_lane<G>();
    const GroupBallot group_ballot = group_ballots<G>();
    const bool want_enc = p.enc || p.enc_cell, want_dec = p.dec || p.dec_cell;
    for (int64_t step = rows_per_round<G>(256), r0 = wave_first_row<G>(256); r0 < nrows; r0 += step) {
        const int64_t r = group_row<G>(r0);
        const bool live = r < nrows;
        const int64_t base = r * p.row_len, ebase = r * (int64_t)p.enc_len, dbase = r * (int64_t)p.dec_len;
        DenoiseCarry carry = denoise_carry_none();
        for (int j0 = 0; j0 < p.row_len; j0 += G) {
            const int j = j0 + lane;
            const bool in = live && j < p.row_len;
            int32_t id = 0;
            bool present = false, eligible = false;
            if (in) {
                const int64_t c = base + j;
                id = p.rows[c];
                const uint8_t mb = p.mask ? p.mask[c] : (uint8_t)1;
                const int32_t sg = p.seg ? p.seg[c] : 1;
                present = denoise_present(mb, sg);
                eligible = mlm_eligible(p.spec.m, id, mb, sg);
            }
            int reach = 0;
            if (eligible) reach = denoise_reach(p.spec, mlm_draw(p.spec.m, r, j), j);
            int x = denoise_scan_pack(denoise_scan_seed(eligible, reach));
#pragma unroll
            for (int d = 1; d < G; d <<= 1) x = denoise_scan_pack(denoise_scan_step(denoise_scan_unpack(x), denoise_scan_unpack(__shfl_up(x, d, G)), lane >= d));
            const int v = denoise_scan_close(denoise_scan_unpack(x), carry.reach);
            const int noise0 = denoise_noise0(v, j) ? 1 : 0;
            int noise0_prev = __shfl_up(noise0, 1, G);
            if (lane == 0) noise0_prev = carry.noise0;
            const bool begin0 = denoise_begin0(noise0 != 0, noise0_prev != 0);
            const uint64_t begin0_lanes = group_ballot(begin0);
            const int run = denoise_run_index(carry, begin0_lanes, lane);
            const bool noise = denoise_noise(p.spec, noise0 != 0, run);
            const bool keep = present && !noise;
            const uint64_t noise_lanes = group_ballot(noise);
            const uint64_t keep_lanes = group_ballot(keep);
            const uint64_t begin_lanes = begin0_lanes & noise_lanes;
            const DenoiseSlots n = denoise_slots(carry, keep_lanes, noise_lanes, begin_lanes, lane);
            const bool begin = begin0 && noise;
            if (keep || begin) {                                      // (never both; both only where `in`)
                const int e = denoise_enc_pos(n);
                if (e < p.enc_len) {
                    if (p.enc) p.enc[ebase + e] = keep ? id : denoise_sentinel(p.spec, run);
                    if (p.enc_cell) p.enc_cell[ebase + e] = keep ? j : -1;
                }
            }
            if (begin) {
                const int d = denoise_dec_sentinel_pos(n);
                if (d < p.dec_len) {
                    if (p.dec) p.dec[dbase + d] = denoise_sentinel(p.spec, run);
                    if (p.dec_cell) p.dec_cell[dbase + d] = -1;
                }
            }
            if (noise) {
                const int d = denoise_dec_pos(n, begin);
                if (d < p.dec_len) {
                    if (p.dec) p.dec[dbase + d] = id;
                    if (p.dec_cell) p.dec_cell[dbase + d] = j;
                }
            }
            carry = denoise_carry_next(carry, __shfl(v, G - 1, G), j0 + G - 1, begin0_lanes, keep_lanes, noise_lanes, begin_lanes);
        }
        if (live) {
            const int ne = denoise_enc_count(carry), nd = denoise_dec_count(p.spec, carry);
            if (want_enc)
                for (int k = ne + lane; k < p.enc_len; k += G) {
                    if (p.enc) p.enc[ebase + k] = p.spec.pad_id;
                    if (p.enc_cell) p.enc_cell[ebase + k] = -1;
                }
            if (want_dec)
                for (int k = nd + lane; k < p.dec_len; k += G) {
                    if (p.dec) p.dec[dbase + k] = p.spec.ignore_label;
                    if (p.dec_cell) p.dec_cell[dbase + k] = -1;
                }
            if (lane == 0) {
                if (p.spec.eos_id >= 0 && nd - 1 < p.dec_len) {
                    if (p.dec) p.dec[dbase + nd - 1] = p.spec.eos_id;
                    if (p.dec_cell) p.dec_cell[dbase + nd - 1] = -1;
                }
                if (p.enc_count) p.enc_count[r] = ne;
                if (p.dec_count) p.dec_count[r] = nd;
                if (p.span_count) p.span_count[r] = carry.begins;
                if ((want_enc && ne > p.enc_len) || (want_dec && nd > p.dec_len)) atomicOr(p.status, 1);
            }
        }
    }
}

void launch_rows_denoise(const RowsDenoiseParams &p, hipStream_t s)
{
    dispatch_span_group(p.row_len, [&](auto g) { hipLaunchKernelGGL((k_rows_denoise<g()>), dim3(rows_grid(p.rows_cap, g())), dim3(256), 0, s, p); });
}

} // namespace bfa
