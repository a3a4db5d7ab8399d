// bf_bucket.h -- length-bucketed batches from ragged ids: a stable sort of the units by width, the sorted list cut into batches under a cell
// budget, every batch padded to its own longest row.
//
// Additive (the reference has no counterpart; include/blingfiretokdll_amd.h IdsToBucketedRowsBatchDevice is the specification).  Sequence q
// becomes the packed stage's unit [cls] ids[0 .. k_q) [sep] of width w_q <= max_len (bf_packed.h PackedSpec with row_len = max_len).  The units
// are ordered by the key max_len - w_q, ties by q: a stable least-significant-digit radix sort, 8 bits a pass, bucket_passes(max_len) passes.
// A batch that starts at sorted position i has rows of L(i) = bucket_row_len cells and holds bucket_count rows; the starts are the chain
// 0, next(0), next(next(0)), ... which the packed stage's pointer doubling marks (bf_packed.h packed_double, packed_rounds).
//
// Everything a lane decides is written once here as BF_HD code: bf_kernels_bucket.hip runs it per lane, tests/hosttest compiles the same header
// for the host (test-only: the product library never sorts on the CPU).  Plain C++, no HIP types.
#pragma once
#include <stdint.h>
#include "bf_packed.h"

namespace bfa {

constexpr int BUCKET_RADIX_BITS = 8, BUCKET_BINS = 1 << BUCKET_RADIX_BITS;
constexpr int BUCKET_THREADS = 256, BUCKET_WAVES = BUCKET_THREADS / 64;
constexpr int BUCKET_TILE = 2048;                     // records a block owns in one pass: a power of two, at most 4096
constexpr int BUCKET_WAVE_TILE = BUCKET_TILE / BUCKET_WAVES, BUCKET_ROUNDS = BUCKET_WAVE_TILE / 64;      // consecutive records of one wave; its rounds of 64
constexpr int BUCKET_FILL_GROUP = 64;                 // sorted positions a wave fills in one visit

struct BucketSpec {
    PackedSpec unit;                      // row_len = max_len
    int max_len, multiple, max_rows;
    int64_t max_cells;
};

// x rounded up to a multiple of m (m >= 1, x >= 0)
BF_HD int64_t bucket_up(int64_t x, int64_t m) { return (x + m - 1) / m * m; }

// fills `s`; false = the parameters are refused (BF_E_ARG).  The flag word is reserved.
BF_HD bool bucket_spec(int max_len, int cls_id, int sep_id, int pad_id, int multiple, int64_t max_cells, int max_rows, int flags, BucketSpec *s)
{
    if (!packed_spec(max_len, cls_id, sep_id, pad_id, flags, &s->unit) || multiple < 1 || max_rows < 0) return false;
    s->max_len = max_len; s->multiple = multiple; s->max_rows = max_rows; s->max_cells = max_cells;
    const int64_t widest = bucket_up(max_len, multiple);                       // (>= multiple: max_len >= 1)
    return max_cells >= widest;
}

// the sort key of a unit of width w: 0 .. max_len, the widest unit first
BF_HD uint32_t bucket_key(const BucketSpec &s, int32_t w) { return (uint32_t)(s.max_len - w); }
BF_HD int32_t bucket_width(const BucketSpec &s, uint32_t key) { return s.max_len - (int32_t)key; }

// passes of 8 bits that cover every key 0 .. max_len: 1 up to 255, 2 up to 65535, 3 above (max_len <= 2^20)
BF_HD int bucket_passes(int max_len)
{
    int bits = 0;
    while (bits < 32 && ((uint32_t)max_len >> bits) != 0) ++bits;
    return (bits + BUCKET_RADIX_BITS - 1) / BUCKET_RADIX_BITS;
}

BF_HD uint32_t bucket_digit(uint32_t key, int pass) { return (key >> (BUCKET_RADIX_BITS * pass)) & (uint32_t)(BUCKET_BINS - 1); }

// blocks of a pass over n records; entry of (digit, block) in the bin-major count array, whose exclusive scan is every block's base for every digit
BF_HD int64_t bucket_blocks(int64_t n) { return (n + BUCKET_TILE - 1) / BUCKET_TILE; }
BF_HD int64_t bucket_count_at(uint32_t digit, int64_t block, int64_t nblocks) { return (int64_t)digit * nblocks + block; }

// Match-any over the digit, one bit at a time: `peers` starts as the ballot of the lanes that hold a record; after the step of bit b it has lost
// the lanes whose digit differs from this lane's in that bit (ballot = the lanes whose bit b is set).  After the eight steps it is the set of
// lanes with this lane's digit; a lane's rank among them is the number of peers below it (mbcnt of the set), their count its population.
BF_HD uint64_t bucket_peers_step(uint64_t peers, uint64_t ballot, uint32_t digit, int bit) { return peers & (((digit >> bit) & 1u) ? ballot : ~ballot); }
BF_HD bool bucket_leader(uint64_t peers, int lane) { return (peers & (((uint64_t)1 << lane) - 1)) == 0; }      // the lowest peer carries the digit's offset on

// cells of a row of the batch whose first (widest) unit has width w: max(multiple, up(w)); at most up(max_len) <= max_cells
BF_HD int32_t bucket_row_len(const BucketSpec &s, int32_t w)
{
    const int64_t u = bucket_up(w, s.multiple);
    return (int32_t)(u > s.multiple ? u : s.multiple);
}

// rows of a batch whose rows have L cells: what the budget takes, at most max_rows (0 = no limit), at least one
BF_HD int64_t bucket_count(const BucketSpec &s, int32_t L)
{
    int64_t n = s.max_cells / L;
    if (s.max_rows > 0 && n > s.max_rows) n = s.max_rows;
    return n < 1 ? 1 : n;
}

// next(i) for i < nseq: one load of the sorted width
BF_HD int32_t bucket_next(const BucketSpec &s, int64_t nseq, int64_t i, int32_t w)
{
    const int64_t n = bucket_count(s, bucket_row_len(s, w));
    return (int32_t)(n < nseq - i ? i + n : nseq);
}

// The first cell of the row of sorted position i in batch b: C_b + (i - first_b) * L_b.  Every position carries its batch's L, and the exclusive
// scan of those over the sorted positions IS that cell (the rows in front of it: whole batches, then the rows of its own batch), so C_b is that
// scan at first_b and no sum over batches is made.  Cell x of the row:
BF_HD int64_t bucket_cell(int64_t row_cell, int32_t x) { return row_cell + x; }

// what cell x of a row whose unit has width w holds; the mask is 1 for every kind but padding.  An id cell of sequence q holds
// ids[off[q] + x - lead]: there are k_q of them, so a sequence whose range was read as empty has none and its ids are never read
enum { BUCKET_CELL_PAD = 0, BUCKET_CELL_CLS, BUCKET_CELL_SEP, BUCKET_CELL_ID };
BF_HD int bucket_cell_kind(const PackedSpec &u, int32_t w, int32_t x)
{
    if (x >= w) return BUCKET_CELL_PAD;
    if (u.lead && x == 0) return BUCKET_CELL_CLS;
    if (u.trail && x == w - 1) return BUCKET_CELL_SEP;
    return BUCKET_CELL_ID;
}

// lanes that share a row in the fill, for rows of `lanes_per_row` lanes: the power of two at or above it, a whole wave beyond 32
BF_HD int bucket_slice(int lanes_per_row)
{
    int s = 1;
    while (s < lanes_per_row && s < 64) s <<= 1;
    return s;
}

} // namespace bfa
