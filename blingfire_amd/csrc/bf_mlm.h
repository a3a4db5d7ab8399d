// bf_mlm.h -- masked-language-model masking of rows that are already there: masked ids and labels, token by token or whole words.
//
// Additive (the reference has no counterpart; include/blingfiretokdll_amd.h RowsMlmMaskBatchDevice is the specification, RowsMlmPredictionsBatchDevice that
// of the cap on a row's predictions at the end of this file).  Every cell of a row
// draws from a counter-based generator keyed by (seed, row, cell, epoch) -- Philox4x32-10 -- so what a cell gets depends on nothing but its
// own coordinates: not on the grid, not on the lane partition, not on the order of calls.  A unit is a cell (token masking) or a run of cells
// whose tokens are byte-adjacent in the text (whole-word masking, over an offset plane pair); the draw of the unit's first cell selects the
// unit, each selected cell's own draw picks its action (mask id / random id / kept).
//
// Everything a cell depends on is written once here as BF_HD code: bf_kernels_mlm.hip runs it per lane, tests/hosttest compiles the same
// header for the host (test-only: the product library never masks on the CPU).  Plain C++, no HIP types.
#pragma once
#include <stdint.h>

#if !defined(BF_HD)
#if defined(__HIPCC__)
#define BF_HD __host__ __device__ __forceinline__
#else
#define BF_HD inline
#endif
#endif

namespace bfa {

constexpr int MLM_MAX_SPECIAL = 8;        // ids that are never masked (BF_MLM_MAX_SPECIAL)
constexpr int MLM_MAX_LEN = 1 << 20;      // row_len above this is refused (ROWS_MAX_LEN)

// ---- Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11): ten rounds, the key bumped after each
struct Philox4 { uint32_t v[4]; };

constexpr uint32_t PHILOX_M0 = 0xD2511F53u, PHILOX_M1 = 0xCD9E8D57u, PHILOX_W0 = 0x9E3779B9u, PHILOX_W1 = 0xBB67AE85u;

BF_HD Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1)
{
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int round = 0; round < 10; ++round) {
        const uint64_t p0 = (uint64_t)PHILOX_M0 * c0, p1 = (uint64_t)PHILOX_M1 * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1; c3 = (uint32_t)p0; c0 = n0; c2 = n2;
        k0 += PHILOX_W0; k1 += PHILOX_W1;
    }
    return Philox4{{c0, c1, c2, c3}};
}

// what a call fixes for all of its cells.  The thresholds are probabilities scaled to 2^32 and compared in 64 bits: 2^32 = always
struct MlmSpec {
    uint64_t t_select, t_mask, t_mask_random;            // Ts, Tm, Tm + Tr
    uint32_t seed_lo, seed_hi, epoch;
    uint32_t rand_span;                                   // rand_hi - rand_lo
    int32_t mask_id, rand_lo, ignore_label;
    int nspecial; int32_t special[MLM_MAX_SPECIAL];
};

// floor(p * 2^32) of a probability; false unless 0 <= p <= 1 (a NaN fails both comparisons)
inline bool mlm_threshold(double p, uint64_t *t)
{
    if (!(p >= 0.0 && p <= 1.0)) return false;
    *t = (uint64_t)(p * 4294967296.0);                    // (exact: a power of two scales the exponent; the cast truncates = floor of a non-negative)
    return true;
}

// fills `s`; false = the parameters are refused (BF_E_ARG).  Host only: the kernels get the finished MlmSpec by value
inline bool mlm_spec(int nspecial, const int32_t *special_ids, double select_prob, double mask_prob, double random_prob, int mask_id, int rand_lo, int rand_hi,
                     int ignore_label, uint64_t seed, uint32_t epoch, MlmSpec *s)
{
    uint64_t tr;
    if (nspecial < 0 || nspecial > MLM_MAX_SPECIAL || (nspecial > 0 && !special_ids)) return false;
    if (!mlm_threshold(select_prob, &s->t_select) || !mlm_threshold(mask_prob, &s->t_mask) || !mlm_threshold(random_prob, &tr)) return false;
    if (!(mask_prob + random_prob <= 1.0)) return false;
    if (tr > 0 && !(0 <= rand_lo && rand_lo < rand_hi)) return false;
    s->t_mask_random = s->t_mask + tr;
    s->seed_lo = (uint32_t)seed; s->seed_hi = (uint32_t)(seed >> 32); s->epoch = epoch;
    s->rand_span = tr > 0 ? (uint32_t)(rand_hi - rand_lo) : 0u;
    s->mask_id = mask_id; s->rand_lo = rand_lo; s->ignore_label = ignore_label;
    s->nspecial = nspecial;
    for (int k = 0; k < MLM_MAX_SPECIAL; ++k) s->special[k] = k < nspecial ? special_ids[k] : 0;
    return true;
}

// W(r, j): the draw of cell j of row r
BF_HD Philox4 mlm_draw(const MlmSpec &s, int64_t r, int j)
{
    return philox4x32_10((uint32_t)(uint64_t)r, (uint32_t)((uint64_t)r >> 32), (uint32_t)j, s.epoch, s.seed_lo, s.seed_hi);
}

// a cell that may be masked: inside the mask, inside a segment, not one of the specials (mask_byte / seg = 1 where the caller has no such plane)
BF_HD bool mlm_eligible(const MlmSpec &s, int32_t id, uint8_t mask_byte, int32_t seg)
{
    bool special = false;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int k = 0; k < MLM_MAX_SPECIAL; ++k) special = special || (k < s.nspecial && id == s.special[k]);
    return mask_byte != 0 && seg != 0 && !special;
}

// ---- units (whole words): cell j continues cell j - 1 when both can join a unit (eligible, start >= 0) and the token of j begins at the byte
// behind the last byte of the token of j - 1 (ends are inclusive).  S - 1 == E, never E + 1 == S: an end of INT32_MAX must not wrap.
BF_HD bool mlm_joins(bool eligible, int32_t start) { return eligible && start >= 0; }

BF_HD bool mlm_continues(bool joins_prev, int32_t end_prev, bool joins, int32_t start) { return joins_prev && joins && start - 1 == end_prev; }

// h(j) = the largest j' <= j that does not continue, as an inclusive max-scan of mlm_head_seed over the cells in order.  A row is walked in chunks
// of G cells (G lanes): the scan runs inside the chunk, a lane that is still at -1 afterwards belongs to the unit that was open at the end of
// the chunk before and takes that chunk's last head.
struct MlmCarry { int32_t end; int joins; int head; };   // of the last cell of the chunk before

BF_HD MlmCarry mlm_carry_none() { return MlmCarry{0, 0, 0}; }   // in front of cell 0: nothing to continue

BF_HD int mlm_head_seed(bool continues, int j) { return continues ? -1 : j; }

// one step of the scan: `up` = the value `d` lanes below, has_up = there is such a lane in the chunk
BF_HD int mlm_head_step(int h, int up, bool has_up) { return has_up && up > h ? up : h; }

BF_HD int mlm_head_close(int h, int carried_head) { return h < 0 ? carried_head : h; }

// ---- the decision for cell j of row r, whose unit begins at cell h: the id and the label it gets
BF_HD void mlm_decide(const MlmSpec &s, int64_t r, int j, int h, int32_t id, bool eligible, int32_t *id_out, int32_t *label_out)
{
    *id_out = id; *label_out = s.ignore_label;
    if (!eligible) return;
    const Philox4 wh = mlm_draw(s, r, h);
    if ((uint64_t)wh.v[0] >= s.t_select) return;
    const Philox4 w = h == j ? wh : mlm_draw(s, r, j);
    *label_out = id;
    if ((uint64_t)w.v[1] < s.t_mask) *id_out = s.mask_id;
    else if ((uint64_t)w.v[1] < s.t_mask_random) *id_out = s.rand_lo + (int32_t)(((uint64_t)w.v[2] * (uint64_t)s.rand_span) >> 32);
}

// ---- the cap on a row's predictions (RowsMlmPredictionsBatchDevice is the specification; k_rows_mlm_cap runs this per lane).  Every cell holds one
// 64-bit word: the key of its unit when the unit is selected, MLM_CAP_NONE otherwise (no key is all ones: a head is below 2^32 - 1).
constexpr int MLM_CAP_MAX_LEN = 4096;               // row_len above this is refused when max_pred > 0 (BF_MLM_CAP_MAX_LEN)
constexpr int MLM_CAP_MAX_PRED = 1 << 20;           // max_pred above this is refused
constexpr uint64_t MLM_CAP_NONE = ~(uint64_t)0;

// K(h) = (W(r, h)[3] << 32) | h
BF_HD uint64_t mlm_cap_key(uint32_t w3, int h) { return ((uint64_t)w3 << 32) | (uint64_t)(uint32_t)h; }

// the word of a cell: the head's draw decides selection (word 0) and carries the key (word 3)
BF_HD uint64_t mlm_cap_word(const MlmSpec &s, bool eligible, const Philox4 &wh, int h)
{
    return eligible && (uint64_t)wh.v[0] < s.t_select ? mlm_cap_key(wh.v[3], h) : MLM_CAP_NONE;
}

// the compare: a cell counts towards g(t) = #{cells : key < t} (MLM_CAP_NONE is below no t)
BF_HD bool mlm_cap_below(uint64_t key, uint64_t t) { return key < t; }

// The threshold search.  g is monotone, T = max { t : g(t) <= P } is built from the high bit down, and a cell is kept iff key < T (a cell with
// key k is kept iff f = g(k + 1) <= P iff k + 1 <= T).  Only bits a key can have are probed: the 32 of W[3] and the hb = ceil(log2 row_len) low bits
// of the head -- bits hb .. 31 of every key are zero, so the largest t with those bits zero separates the keys exactly as the largest t does
// (were a key k with T <= k kept, k + 1 or, past the last head of its high word, (hi + 1) << 32 would be a larger such t).  That argument needs a
// key behind T, so the search is run only where the row's selected cells exceed P; where they do not, every selected cell is kept.
BF_HD int mlm_cap_head_bits(int row_len) { int b = 0; while (((int64_t)1 << b) < row_len) ++b; return b; }

BF_HD int mlm_cap_rounds(int head_bits) { return 32 + head_bits; }

// round i = rounds - 1 .. 0 probes T with one more bit set
BF_HD uint64_t mlm_cap_probe(uint64_t T, int i, int head_bits) { return T | ((uint64_t)1 << (i < head_bits ? i : i - head_bits + 32)); }

// n = g(probe): the probe becomes T when it still fits
BF_HD uint64_t mlm_cap_take(uint64_t T, uint64_t probe, int n, int P) { return n <= P ? probe : T; }

// kept: selected, and uncapped (P = 0), or the whole row fits, or in front of the threshold
BF_HD bool mlm_cap_kept(uint64_t key, int selected_cells, int P, uint64_t T) { return key != MLM_CAP_NONE && (P == 0 || selected_cells <= P || key < T); }

// the gather slot of a kept cell = the kept cells in front of it: those of the chunks before (the carry) and those of the lanes below it in its
// own chunk.  `kept_lanes` has bit l set when lane l of the cell's group keeps its cell (the group's bits of a ballot, shifted down to bit 0).
struct MlmCapCarry { int kept; };

BF_HD MlmCapCarry mlm_cap_carry_none() { return MlmCapCarry{0}; }

BF_HD int mlm_popcount64(uint64_t x)
{
    return __builtin_popcountll(x);
}

BF_HD int mlm_cap_slot(MlmCapCarry carry, uint64_t kept_lanes, int lane) { return carry.kept + mlm_popcount64(kept_lanes & (((uint64_t)1 << lane) - 1)); }

BF_HD MlmCapCarry mlm_cap_carry_next(MlmCapCarry carry, uint64_t kept_lanes) { return MlmCapCarry{carry.kept + mlm_popcount64(kept_lanes)}; }

// what a kept cell puts into ids: its own draw picks the action, as in mlm_decide
BF_HD int32_t mlm_kept_id(const MlmSpec &s, int64_t r, int j, int32_t id)
{
    const Philox4 w = mlm_draw(s, r, j);
    if ((uint64_t)w.v[1] < s.t_mask) return s.mask_id;
    if ((uint64_t)w.v[1] < s.t_mask_random) return s.rand_lo + (int32_t)(((uint64_t)w.v[2] * (uint64_t)s.rand_span) >> 32);
    return id;
}

} // namespace bfa
