// bf_pairs.h -- fixed-shape model inputs from pairs of ragged id sequences: a pair's geometry, its row count and the cell of a row.
//
// Additive (the reference has no counterpart; include/blingfiretokdll_amd.h IdsToPairRowsBatchDevice is the specification).  Pair q is
// A (na ids) and B (nb ids); a row is
//     [cls] A' [sep]([sep]) B' [sep] pad...                                 (flag bit 0: the padding comes first; bit 1: two middle separators)
// of row_len cells with a mask (1 over everything but the padding) and a type byte (1 over B' and the trailing separator).  T = row_len -
// specials is the room for ids.
//   mode 0   A' = the first ka = min(na, max_a) ids of A in every row; B is cut into windows of body_b = T - ka ids whose starts lie
//            step = body_b - stride apart: the geometry is the pair's own, because ka is.
//   mode 1   one row: ids leave the end of the longer sequence (B on a tie) until ka + kb <= T, in closed form.
//
// Everything a cell depends on is written once here as BF_HD code: bf_kernels_pairs.hip runs it per lane, tests/hosttest compiles the same
// header for the host (test-only: the product library never fills rows on the CPU).  Plain C++, no HIP types.
#pragma once
#include "bf_rows.h"

namespace bfa {

constexpr int PAIRS_PAD_LEFT = 1;         // flags bit 0
constexpr int PAIRS_DOUBLE_SEP = 2;       // flags bit 1

// what a cell holds, beside ROWS_CELL_PAD / ROWS_CELL_CLS / ROWS_CELL_SEP
constexpr int PAIRS_CELL_A = 0, PAIRS_CELL_B = 1;

struct PairsSpec {
    int row_len, cls_id, sep_id, pad_id;
    int lead, mid, trail;                 // cells of cls_id; of sep_id between A' and B' (0, 1 or 2); of sep_id behind B'
    int room;                             // T: ids a row holds
    int mode, max_a, stride;
    int max_rows;                         // rows kept per pair; 0 = all
    int pad_left;
};

// fills `s`; false = the parameters are refused (BF_E_ARG)
BF_HD bool pairs_spec(int row_len, int cls_id, int sep_id, int pad_id, int mode, int max_a, int stride, int max_rows_per_pair, int flags, PairsSpec *s)
{
    if (row_len < 1 || row_len > ROWS_MAX_LEN || (mode != 0 && mode != 1) || (flags & ~(PAIRS_PAD_LEFT | PAIRS_DOUBLE_SEP)) != 0) return false;
    if ((flags & PAIRS_DOUBLE_SEP) && sep_id < 0) return false;
    s->row_len = row_len; s->cls_id = cls_id; s->sep_id = sep_id; s->pad_id = pad_id;
    s->lead = cls_id >= 0 ? 1 : 0; s->trail = sep_id >= 0 ? 1 : 0;
    s->mid = sep_id >= 0 ? ((flags & PAIRS_DOUBLE_SEP) ? 2 : 1) : 0;
    s->room = row_len - s->lead - s->mid - s->trail;
    if (s->room < 1) return false;
    if (mode == 0 ? (max_a < 0 || max_a > s->room - 1 || stride < 0 || stride >= s->room - max_a || max_rows_per_pair < 0)
                  : (max_a != 0 || stride != 0 || max_rows_per_pair != 1)) return false;
    s->mode = mode; s->max_a = max_a; s->stride = stride; s->max_rows = max_rows_per_pair;
    s->pad_left = (flags & PAIRS_PAD_LEFT) ? 1 : 0;
    return true;
}

// a pair's own geometry: ids of A in every row, ids of B a row has room for, distance of two window starts (all >= 1 but ka, and body_b in mode 1)
struct PairGeom { int ka, body_b, step; };

BF_HD PairGeom pairs_geom(const PairsSpec &s, int64_t na, int64_t nb)
{
    PairGeom g;
    if (s.mode == 0) {
        g.ka = (int)(na < s.max_a ? na : s.max_a);
        g.body_b = s.room - g.ka;
        g.step = g.body_b - s.stride;
    } else {
        // dropping one id at a time from the end of the longer sequence (B on a tie) until both fit leaves A the larger half of the room, and
        // whatever B does not need
        const int64_t half = (s.room + 1) / 2, spare = s.room - nb;
        const int64_t keep = half > spare ? half : spare;
        g.ka = (int)(na < keep ? na : keep);
        g.body_b = s.room - g.ka;
        g.step = g.body_b > 0 ? g.body_b : 1;      // (unused: one row)
    }
    return g;
}

// rows of a pair; a count beyond INT32_MAX saturates (*saturated is set then)
BF_HD int32_t pairs_count(const PairsSpec &s, const PairGeom &g, int64_t nb, bool *saturated)
{
    *saturated = false;
    if (s.mode != 0 || nb <= g.body_b) return 1;
    int64_t rows = 1 + (nb - g.body_b + g.step - 1) / g.step;
    if (s.max_rows > 0 && rows > s.max_rows) rows = s.max_rows;
    if (rows > 0x7fffffff) { rows = 0x7fffffff; *saturated = true; }
    return (int32_t)rows;
}

// one row per pair whatever the lengths: row r is pair r and starts at the first id of B (no search, nothing to look up)
BF_HD bool pairs_one_row(const PairsSpec &s) { return s.mode != 0 || s.max_rows == 1; }

// a cell: which sequence it reads (PAIRS_CELL_A / _B, `at` = the index of the id within it) or ROWS_CELL_*; its type byte
struct PairCell { int64_t at; int what; uint8_t type; };

// a row laid out once for all of its cells: behind `shift` cells of padding in front, cls | A' = [a0, a1) | separators | B' = [b0, b1) | the
// trailing separator end at `real`
struct PairRow { int shift, a0, a1, b0, b1, real; int64_t first_b; };

// the row of a pair (nb ids in B; geometry g) whose first B id is number first_b of B
BF_HD PairRow pairs_row(const PairsSpec &s, const PairGeom &g, int64_t first_b, int64_t nb)
{
    int64_t kb = nb - first_b;            // ids of B in this row
    if (kb > g.body_b) kb = g.body_b;
    if (kb < 0) kb = 0;
    PairRow w;
    w.a0 = s.lead; w.a1 = w.a0 + g.ka; w.b0 = w.a1 + s.mid; w.b1 = w.b0 + (int)kb; w.real = w.b1 + s.trail;
    w.shift = s.pad_left ? s.row_len - w.real : 0;
    w.first_b = first_b;
    return w;
}

// cell j (0 .. row_len - 1) of a row (written as selections, not as branches: a lane does this four times per store)
BF_HD PairCell pairs_cell(const PairRow &w, int j)
{
    const int x = j - w.shift;
    const bool in_a = x >= w.a0 && x < w.a1, in_b = x >= w.b0 && x < w.b1, real = x >= 0 && x < w.real;
    PairCell c;
    c.what = in_a ? PAIRS_CELL_A : in_b ? PAIRS_CELL_B : (int)(!real ? ROWS_CELL_PAD : x < w.a0 ? ROWS_CELL_CLS : ROWS_CELL_SEP);
    c.at = in_b ? w.first_b + (x - w.b0) : (int64_t)(x - w.a0);      // (read for an id only)
    c.type = real && x >= w.b0 ? 1 : 0;
    return c;
}

static_assert(PAIRS_CELL_A == CELL_SIDE_A && PAIRS_CELL_B == CELL_SIDE_B, "a pair cell's `what` is the side of its CellWhere");
// pairs_cell as a CellWhere (bf_rows.h): side = PAIRS_CELL_A / PAIRS_CELL_B and the index within that sequence, or side < 0
BF_HD CellWhere pairs_where(const PairRow &w, int j)
{
    const PairCell c = pairs_cell(w, j);
    return CellWhere{c.at, c.what >= 0 ? c.what : -1};
}

// the id, the mask byte and the type byte of a cell; seq_a / seq_b = the ids of its pair
BF_HD int32_t pairs_cell_value(const PairsSpec &s, const PairCell &c, const int32_t *seq_a, const int32_t *seq_b, uint8_t *mask, uint8_t *type)
{
    *mask = c.what == (int)ROWS_CELL_PAD ? 0 : 1;
    *type = c.type;
    int32_t v = c.what == (int)ROWS_CELL_CLS ? s.cls_id : c.what == (int)ROWS_CELL_SEP ? s.sep_id : s.pad_id;
    if (c.what >= 0) v = (c.what == PAIRS_CELL_B ? seq_b : seq_a)[c.at];          // (one load, whichever side)
    return v;
}

// The pair stage's source (what a source supplies: bf_rows.h RowsSource): items that are one range of each of two id arrays.  An item carries
// its own geometry; a row's first id is a B id.
struct PairsSource {
    static constexpr bool HAS_TYPE = true;
    PairsSpec spec;
    const int32_t *ids_a, *ids_b; int64_t len_a, len_b; const int64_t *off_a, *off_b;      // pair q = A: ids_a[off_a[q] .. off_a[q+1]), B likewise

    struct Item { const int32_t *seq_a, *seq_b; int64_t nb; PairGeom g; bool bad; };
    typedef PairRow Row;

    BF_HD bool valid() const { return len_a >= 0 && len_b >= 0 && off_a && off_b && (len_a == 0 || ids_a) && (len_b == 0 || ids_b); }
    BF_HD Item load(int64_t q) const
    {
        Item it;
        bool bad_a, bad_b;
        const int64_t a0 = off_a[q], b0 = off_b[q];
        const int64_t na = rows_seq_len(a0, off_a[q + 1], len_a, &bad_a);
        it.nb = rows_seq_len(b0, off_b[q + 1], len_b, &bad_b);
        it.seq_a = ids_a + (bad_a ? 0 : a0); it.seq_b = ids_b + (bad_b ? 0 : b0);
        it.g = pairs_geom(spec, na, it.nb);
        it.bad = bad_a || bad_b;
        return it;
    }
    BF_HD int32_t count(const Item &it, bool *saturated) const { return pairs_count(spec, it.g, it.nb, saturated); }
    BF_HD bool one_row() const { return pairs_one_row(spec); }
    BF_HD int64_t first(const Item &it, int64_t k) const { return spec.mode == 0 ? k * it.g.step : 0; }
    BF_HD Row row(const Item &it, int64_t first) const { return pairs_row(spec, it.g, first, it.nb); }
    BF_HD int32_t cell(const Item &it, const Row &w, int j, uint8_t *mask, uint8_t *type) const
    {
        return pairs_cell_value(spec, pairs_cell(w, j), it.seq_a, it.seq_b, mask, type);
    }
    BF_HD CellWhere where(const Item &it, const Row &w, int j) const
    {
        CellWhere c = pairs_where(w, j);
        c.at += c.side == CELL_SIDE_B ? it.seq_b - ids_b : it.seq_a - ids_a;
        return c;
    }
};

} // namespace bfa
