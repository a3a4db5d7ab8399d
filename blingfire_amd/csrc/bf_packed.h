// bf_packed.h -- packed rows from ragged ids: several sequences share a row, a segment plane and a position plane tell them apart.
//
// Additive (the reference has no counterpart; include/blingfiretokdll_amd.h IdsToPackedRowsBatchDevice is the specification).  Sequence q
// becomes the unit [cls] ids[0 .. k_q) [sep] of width w_q <= row_len; W = the exclusive scan of the widths.  A row that starts at sequence s
// holds the sequences [s, next(s)), next(s) = the largest e in (s, nseq] with W[e] - W[s] <= row_len, and the next row starts there: the row
// starts are the chain 0, next(0), next(next(0)), ...  No lane walks it: the sequences on the chain are marked by pointer doubling
// (packed_double, packed_rounds(nseq) rounds over the whole array), a scan of the marks numbers the rows.
//
// Everything a lane decides is written once here as BF_HD code: bf_kernels_packed.hip runs it per lane, tests/hosttest compiles the same
// header for the host (test-only: the product library never packs rows on the CPU).  Plain C++, no HIP types.
#pragma once
#include <stdint.h>
#include "bf_rows.h"

namespace bfa {

struct PackedSpec {
    int row_len, cls_id, sep_id, pad_id;
    int body;                             // ids a unit holds at most
    int lead, trail;                      // 1 when cls_id / sep_id are written
};

// fills `s`; false = the parameters are refused (BF_E_ARG).  The flag word is reserved.
BF_HD bool packed_spec(int row_len, int cls_id, int sep_id, int pad_id, int flags, PackedSpec *s)
{
    if (row_len < 1 || row_len > ROWS_MAX_LEN || flags != 0) return false;
    s->row_len = row_len; s->cls_id = cls_id; s->sep_id = sep_id; s->pad_id = pad_id;
    s->lead = cls_id >= 0 ? 1 : 0; s->trail = sep_id >= 0 ? 1 : 0;
    s->body = row_len - s->lead - s->trail;
    return s->body >= 1;
}

// the width of the unit of a sequence of n ids (n as rows_seq_len gives it): 0 .. row_len
BF_HD int32_t packed_width(const PackedSpec &s, int64_t n) { return (int32_t)(s.lead + (n < s.body ? n : s.body) + s.trail); }

// next(s) for s < nseq: the largest e in (s, nseq] with W[e] - W[s] <= row_len (e = s + 1 always qualifies: no unit is wider than a row).
// An upper-bound search that gallops from s + 1, since a row ends a few units behind its start unless it runs into units of width 0.
BF_HD int32_t packed_next(const int64_t *W, int64_t nseq, int64_t s, int row_len)
{
    const int64_t target = W[s] + row_len;
    int64_t lo = s + 1, step = 1;
    while (lo + step <= nseq && W[lo + step] <= target) { lo += step; step <<= 1; }
    int64_t hi = lo + step <= nseq ? lo + step : nseq + 1;        // the first candidate known not to qualify (or past the end)
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (W[mid] <= target) lo = mid; else hi = mid;
    }
    return (int32_t)lo;
}

// doubling rounds that mark every sequence the chain from 0 visits: ceil(log2(nseq + 1)).  After round k (from 0) the first 2^(k+1) chain
// nodes are marked and the jump array holds next applied 2^(k+1) times; the chain has at most nseq + 1 nodes (nseq itself is the last).
BF_HD int packed_rounds(int64_t nseq)
{
    int k = 0;
    while (((int64_t)1 << k) < nseq + 1) ++k;
    return k;
}

// one lane of one round, s in [0, nseq]: a marked s marks jin[s]; the jump of s is squared into the other buffer.  Every writer of a mark
// writes 1, and a mark another lane of the same round set early only marks a further chain node: no ordering inside a round is needed.
BF_HD void packed_double(const int32_t *jin, int32_t *jout, int32_t *mark, int64_t s)
{
    const int32_t j = jin[s];
    if (mark[s]) mark[j] = 1;
    jout[s] = jin[j];
}

// the unit of a cell: the last q in [s, e) with W[q] <= target (s qualifies).  Units of width 0 share their W with the unit behind them, so
// the last one is the unit the cell lies in.
BF_HD int64_t packed_find_unit(const int64_t *W, int64_t s, int64_t e, int64_t target)
{
    int64_t lo = s, hi = e;
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (W[mid] <= target) lo = mid; else hi = mid;
    }
    return lo;
}

struct PackedCell { int32_t id, seg, pos; };

BF_HD PackedCell packed_pad_cell(const PackedSpec &sp) { return PackedCell{sp.pad_id, 0, 0}; }

// Where a cell reads.  The fill (packed_cell) and the companion planes (packed_where, k_packed_planes) find a cell's unit by the same steps and
// name the element it holds by the same call:
//   packed_locate  the unit the cell lies in and its place there, or "padding" -- packed_cell keeps these five lines in its own body, word for
//                  word: routed through the call, k_packed_fill<4> compiled to 15 % more instructions and the base call ran slower than the parent's
//   packed_id_at   for a place that holds an id, that id's element of the ids -- and of every array parallel to them
// A unit's first place holds cls_id when there is a lead, its last one sep_id when there is a trail, every other place an id.
// tests/hosttest/bf_packedplanestest.cpp holds the two to each other cell by cell: where packed_cell fetched ids[i], packed_where says i.

// cell j of the row [s, e) (s = f[r], e = f[r + 1]): false = padding; else *q_io is the cell's unit, *w its width and *x the cell's place in it.
// *q_io comes in as a unit of the row at or in front of the cell's (s to begin with): a lane that fills cells from left to right searches
// only where the cell left the unit of the cell before
BF_HD bool packed_locate(const int64_t *W, int64_t s, int64_t e, int j, int64_t *q_io, int32_t *w, int32_t *x)
{
    const int64_t base = W[s], target = base + j;
    if (target >= W[e]) return false;
    int64_t q = *q_io;
    if (W[q + 1] <= target) q = packed_find_unit(W, q + 1, e, target);
    *q_io = q;
    *w = (int32_t)(W[q + 1] - W[q]); *x = (int32_t)(target - W[q]);
    return true;
}

// the element that place x of the unit of sequence q holds, for a place that holds an id: the sequence's range is good then (a bad range is read
// as empty: its unit has no such place), so the index is inside [0, ids_len)
BF_HD int64_t packed_id_at(const PackedSpec &sp, int64_t q, int32_t x, const int64_t *id_off) { return id_off[q] + x - sp.lead; }

// cell x of the unit of sequence q (width w > x) in the row that starts at sequence s
BF_HD PackedCell packed_unit_cell(const PackedSpec &sp, int64_t s, int64_t q, int32_t w, int32_t x, const int32_t *ids, const int64_t *id_off)
{
    PackedCell c;
    c.seg = (int32_t)(q - s + 1); c.pos = x;
    if (sp.lead && x == 0) c.id = sp.cls_id;
    else if (sp.trail && x == w - 1) c.id = sp.sep_id;
    else c.id = ids[packed_id_at(sp, q, x, id_off)];
    return c;
}

// cell j of the row [s, e); *q_io as in packed_locate, whose steps these are
BF_HD PackedCell packed_cell(const PackedSpec &sp, const int64_t *W, int64_t s, int64_t e, int j, const int32_t *ids, const int64_t *id_off, int64_t *q_io)
{
    const int64_t base = W[s], target = base + j;
    if (target >= W[e]) return packed_pad_cell(sp);
    int64_t q = *q_io;
    if (W[q + 1] <= target) q = packed_find_unit(W, q + 1, e, target);
    *q_io = q;
    return packed_unit_cell(sp, s, q, (int32_t)(W[q + 1] - W[q]), (int32_t)(target - W[q]), ids, id_off);
}

// the element index of the id that cell j of the row [s, e) holds, PACKED_NONE where it holds cls_id, sep_id or padding: packed_cell with the
// fetch left out (what a companion plane gathers by)
constexpr int64_t PACKED_NONE = -1;
BF_HD int64_t packed_where(const PackedSpec &sp, const int64_t *W, int64_t s, int64_t e, int j, const int64_t *id_off, int64_t *q_io)
{
    int32_t w, x;
    if (!packed_locate(W, s, e, j, q_io, &w, &x)) return PACKED_NONE;
    if ((sp.lead && x == 0) || (sp.trail && x == w - 1)) return PACKED_NONE;
    return packed_id_at(sp, *q_io, x, id_off);
}

} // namespace bfa
