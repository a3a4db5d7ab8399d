// bf_denoise.h -- span corruption (the denoising objective of the T5 / mT5 / UL2 family) of rows that are already there: an encoder row in which
// every noise run has collapsed to one sentinel, and a decoder row that lists the runs behind their sentinels.
//
// Additive (the reference has no counterpart; include/blingfiretokdll_amd.h RowsDenoiseBatchDevice is the specification).  Every eligible cell draws
// W(r, j) of bf_mlm.h once: word 0 decides whether a span starts at the cell, word 1 how long it is.  A cell is raw noise when a span that started
// at or in front of it, with nothing ineligible between, still covers it; that is an inclusive max-scan of the spans' reaches (start + length)
// that an ineligible cell resets -- a segmented scan.  Runs of raw noise are numbered by a count of their first cells, the cap on the sentinels
// turns the runs past it back into copied cells, and three running counts (kept cells, noise cells, run begins) give every cell its place in
// the two compacted rows.
//
// Everything a cell depends on is written once here as BF_HD code: bf_kernels_denoise.hip runs it per lane, tests/hosttest compiles the same
// header for the host (test-only: the product library never corrupts spans on the CPU).  Plain C++, no HIP types.
#pragma once
#include <stdint.h>
#include "bf_mlm.h"

namespace bfa {

constexpr int DENOISE_MAX_LEN = 1 << 20;        // row_len, enc_len, dec_len, len_hi and max_sentinels above this are refused

// what a call fixes for all of its cells
struct DenoiseSpec {
    MlmSpec m;                                   // the generator key, the epoch and the specials: what mlm_draw and mlm_eligible read (the rest is zero)
    uint64_t t_start;                            // Ts = floor(start_prob * 2^32), compared in 64 bits: 2^32 = every eligible cell starts
    int32_t len_lo; uint32_t len_span;           // len = len_lo + ((W[1] * len_span) >> 32), len_span = len_hi - len_lo + 1
    int32_t sentinel_first, sentinel_step, max_sentinels;
    int32_t eos_id, pad_id, ignore_label;
};

// fills `s`; false = the parameters are refused (BF_E_ARG).  Host only: the kernel gets the finished DenoiseSpec by value
inline bool denoise_spec(int nspecial, const int32_t *special_ids, double start_prob, int len_lo, int len_hi, int sentinel_first, int sentinel_step, int max_sentinels,
                         int eos_id, int pad_id, int ignore_label, uint64_t seed, uint32_t epoch, DenoiseSpec *s)
{
    if (!mlm_spec(nspecial, special_ids, 0.0, 0.0, 0.0, 0, 0, 0, ignore_label, seed, epoch, &s->m)) return false;
    if (!mlm_threshold(start_prob, &s->t_start)) return false;
    if (!(1 <= len_lo && len_lo <= len_hi && len_hi <= DENOISE_MAX_LEN)) return false;
    if (max_sentinels < 1 || max_sentinels > DENOISE_MAX_LEN) return false;
    const int64_t last = (int64_t)sentinel_first + (int64_t)(max_sentinels - 1) * (int64_t)sentinel_step;
    if (sentinel_first < 0 || last < 0 || last > (int64_t)INT32_MAX) return false;
    s->len_lo = len_lo; s->len_span = (uint32_t)(len_hi - len_lo + 1);
    s->sentinel_first = sentinel_first; s->sentinel_step = sentinel_step; s->max_sentinels = max_sentinels;
    s->eos_id = eos_id; s->pad_id = pad_id; s->ignore_label = ignore_label;
    return true;
}

// a cell that reaches an output at all: inside the mask, inside a segment (mask_byte / seg = 1 where the caller has no such plane)
BF_HD bool denoise_present(uint8_t mask_byte, int32_t seg) { return mask_byte != 0 && seg != 0; }

// the reach of an eligible cell j with draw w: one past the last cell its span covers, 0 where no span starts (j + len <= 2^21: no wrap)
BF_HD int denoise_reach(const DenoiseSpec &s, const Philox4 &w, int j)
{
    const bool starts = (uint64_t)w.v[0] < s.t_start;
    const int len = s.len_lo + (int)(((uint64_t)w.v[1] * (uint64_t)s.len_span) >> 32);
    return starts ? j + len : 0;
}

// ---- the segmented inclusive max-scan of the reach.  An element is (f, v): f = an ineligible cell lies in the stretch the element stands for,
// v = the largest reach behind the last such cell.  (f, v) o (f', v') = (f | f', f' ? v' : max(v, v')), the left operand being the cells in front.
// A row is walked in chunks of G cells (G lanes): the scan runs inside the chunk, and a lane with no ineligible cell at or below it in its chunk
// also takes what the last cell of the chunk before carried.
struct DenoiseScan { int f, v; };

BF_HD DenoiseScan denoise_scan_seed(bool eligible, int reach) { return DenoiseScan{eligible ? 0 : 1, eligible ? reach : 0}; }

// one step of the scan: `up` = the element `d` lanes below, has_up = there is such a lane in the chunk
BF_HD DenoiseScan denoise_scan_step(DenoiseScan s, DenoiseScan up, bool has_up)
{
    if (!has_up) return s;
    return DenoiseScan{s.f | up.f, s.f ? s.v : (up.v > s.v ? up.v : s.v)};
}

// an element as one word, so that a step of the scan moves one register across the lanes: the reach is below 2^22 (DENOISE_MAX_LEN twice)
BF_HD int denoise_scan_pack(DenoiseScan s) { return (s.f << 30) | s.v; }

BF_HD DenoiseScan denoise_scan_unpack(int x) { return DenoiseScan{x >> 30, x & ((1 << 30) - 1)}; }

BF_HD int denoise_scan_close(DenoiseScan s, int carried_reach) { return s.f ? s.v : (carried_reach > s.v ? carried_reach : s.v); }

// raw noise: a span that nothing ineligible cut still covers cell j (an ineligible cell has v = 0)
BF_HD bool denoise_noise0(int v, int j) { return v > j; }

// a run begins where raw noise follows a cell that is none (the cell one lane up; lane 0: the carry)
BF_HD bool denoise_begin0(bool noise0, bool noise0_prev) { return noise0 && !noise0_prev; }

// what the chunks in front of a chunk hand on: the closed reach and the raw-noise flag of their last cell, the runs begun (capped or not), and
// the three running counts of the capped result
struct DenoiseCarry { int reach, noise0, runs, keep, noise, begins; };

BF_HD DenoiseCarry denoise_carry_none() { return DenoiseCarry{0, 0, 0, 0, 0, 0}; }   // in front of cell 0: no span, no run, nothing counted

BF_HD uint64_t denoise_lanes_below(int lane) { return ((uint64_t)1 << lane) - 1; }

// the index of the run a raw-noise cell belongs to: the begins at or below its lane (its own included) and those of the chunks before, less one.
// `begin0_lanes` has bit l set when lane l of the cell's group begins a run (the group's bits of a ballot, shifted down to bit 0)
BF_HD int denoise_run_index(const DenoiseCarry &c, uint64_t begin0_lanes, int lane)
{
    return c.runs + mlm_popcount64(begin0_lanes & denoise_lanes_below(lane)) + (int)((begin0_lanes >> lane) & 1) - 1;
}

// the cap: a run past the last sentinel is not noise
BF_HD bool denoise_noise(const DenoiseSpec &s, bool noise0, int run) { return noise0 && run < s.max_sentinels; }

BF_HD int32_t denoise_sentinel(const DenoiseSpec &s, int run) { return s.sentinel_first + run * s.sentinel_step; }

// the running counts in front of a lane's cell: ballot + popcount slots with a carry, as mlm_cap_slot
struct DenoiseSlots { int keep, noise, begins; };

BF_HD DenoiseSlots denoise_slots(const DenoiseCarry &c, uint64_t keep_lanes, uint64_t noise_lanes, uint64_t begin_lanes, int lane)
{
    const uint64_t below = denoise_lanes_below(lane);
    return DenoiseSlots{c.keep + mlm_popcount64(keep_lanes & below), c.noise + mlm_popcount64(noise_lanes & below), c.begins + mlm_popcount64(begin_lanes & below)};
}

// (last_reach, last_cell: the closed reach and the index of the chunk's last cell, which say whether that cell is raw noise)
BF_HD DenoiseCarry denoise_carry_next(const DenoiseCarry &c, int last_reach, int last_cell, uint64_t begin0_lanes, uint64_t keep_lanes, uint64_t noise_lanes,
                                      uint64_t begin_lanes)
{
    return DenoiseCarry{last_reach, denoise_noise0(last_reach, last_cell) ? 1 : 0, c.runs + mlm_popcount64(begin0_lanes), c.keep + mlm_popcount64(keep_lanes), c.noise + mlm_popcount64(noise_lanes),
                        c.begins + mlm_popcount64(begin_lanes)};
}

// ---- the two output positions.  Encoder: a kept cell, or the sentinel of a run's first cell, stands behind the kept cells and the begins in front
// of it.  Decoder: a sentinel stands behind the noise cells and the begins in front of its run's first cell, a noise cell one further when it is
// that first cell itself (begins at or below it).
BF_HD int denoise_enc_pos(const DenoiseSlots &n) { return n.keep + n.begins; }

BF_HD int denoise_dec_sentinel_pos(const DenoiseSlots &n) { return n.noise + n.begins; }

BF_HD int denoise_dec_pos(const DenoiseSlots &n, bool begin) { return n.noise + n.begins + (begin ? 1 : 0); }

// the untruncated lengths of a finished row
BF_HD int denoise_enc_count(const DenoiseCarry &c) { return c.keep + c.begins; }

BF_HD int denoise_dec_count(const DenoiseSpec &s, const DenoiseCarry &c) { return c.noise + c.begins + (s.eos_id >= 0 ? 1 : 0); }

} // namespace bfa
