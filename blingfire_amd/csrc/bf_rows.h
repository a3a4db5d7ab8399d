// bf_rows.h -- fixed-shape model inputs from ragged ids: the window count of a sequence and the cell of a row.
//
// Additive (the reference has no counterpart; include/blingfiretokdll_amd.h IdsToRowsBatchDevice is the specification).  A sequence of n
// ids is cut into windows of `body` ids whose starts lie `step` = body - stride apart; window w becomes the row
//     [cls] ids[w * step .. min(n, w * step + body)) [sep] pad...          (flag bit 0: the padding comes first)
// of row_len cells, with a mask that is 1 over the real cells.  A sequence that fits (n <= body; an empty one too) has one row.
//
// Everything a cell depends on is written once here as BF_HD code: bf_kernels_rows.hip runs it per lane, tests/hosttest compiles the same
// header for the host (test-only: the product library never fills rows on the CPU).  Plain C++, no HIP types.
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

constexpr int ROWS_MAX_LEN = 1 << 20;     // row_len above this is refused
constexpr int ROWS_PAD_LEFT = 1;          // flags bit 0

// what a cell holds: an index into its sequence (>= 0) or one of these
constexpr int64_t ROWS_CELL_PAD = -1, ROWS_CELL_CLS = -2, ROWS_CELL_SEP = -3;

struct RowsSpec {
    int row_len, cls_id, sep_id, pad_id;
    int body, step;                       // ids per window; distance of two window starts
    int lead, trail;                      // 1 when cls_id / sep_id are written
    int max_rows;                         // windows kept per sequence; 0 = all
    int pad_left;
};

// fills `s`; false = the parameters are refused (BF_E_ARG)
BF_HD bool rows_spec(int row_len, int cls_id, int sep_id, int pad_id, int stride, int max_rows_per_seq, int flags, RowsSpec *s)
{
    if (row_len < 1 || row_len > ROWS_MAX_LEN || max_rows_per_seq < 0 || (flags & ~ROWS_PAD_LEFT) != 0) return false;
    s->row_len = row_len; s->cls_id = cls_id; s->sep_id = sep_id; s->pad_id = pad_id;
    s->lead = cls_id >= 0 ? 1 : 0; s->trail = sep_id >= 0 ? 1 : 0;
    s->body = row_len - s->lead - s->trail;
    if (s->body < 1 || stride < 0 || stride >= s->body) return false;
    s->step = s->body - stride;
    s->max_rows = max_rows_per_seq; s->pad_left = (flags & ROWS_PAD_LEFT) ? 1 : 0;
    return true;
}

// ids of sequence q as the kernels see it: 0 when its range is not inside [0, ids_len] or its offsets decrease (*bad is set then)
BF_HD int64_t rows_seq_len(int64_t b, int64_t e, int64_t ids_len, bool *bad)
{
    *bad = b < 0 || e < b || e > ids_len;
    return *bad ? 0 : e - b;
}

// rows of a sequence of n ids; a count beyond INT32_MAX saturates (*saturated is set then)
BF_HD int32_t rows_count(const RowsSpec &s, int64_t n, bool *saturated)
{
    *saturated = false;
    if (n <= s.body) return 1;
    int64_t rows = 1 + (n - s.body + s.step - 1) / s.step;
    if (s.max_rows > 0 && rows > s.max_rows) rows = s.max_rows;
    if (rows > 0x7fffffff) { rows = 0x7fffffff; *saturated = true; }
    return (int32_t)rows;
}

// cell j (0 .. row_len - 1) of the row whose first id is number row_first of a sequence of n ids: the index of the id it holds, or ROWS_CELL_*
BF_HD int64_t rows_cell(const RowsSpec &s, int64_t row_first, int64_t n, int j)
{
    int64_t k = n - row_first;            // ids in this window
    if (k > s.body) k = s.body;
    if (k < 0) k = 0;
    const int real = (int)k + s.lead + s.trail;
    const int x = s.pad_left ? j - (s.row_len - real) : j;
    if (x < 0 || x >= real) return ROWS_CELL_PAD;
    if (s.lead && x == 0) return ROWS_CELL_CLS;
    const int i = x - s.lead;
    return i < k ? row_first + i : ROWS_CELL_SEP;
}

// where a cell reads: `side` = the id array (0; bf_pairs.h: PAIRS_CELL_A / PAIRS_CELL_B) and `at` = the index of the element in it, or
// side < 0 = the cell holds no id (a special or padding).  What the companion planes gather by (k_rowstage_planes).
struct CellWhere { int64_t at; int side; };
constexpr int CELL_SIDE_A = 0, CELL_SIDE_B = 1;          // the sides there are: the first index of RowPlanesParams::src (a source with one id array has side A alone)

// rows_cell as a CellWhere: `at` = the index within the sequence
BF_HD CellWhere rows_where(const RowsSpec &s, int64_t row_first, int64_t n, int j)
{
    const int64_t c = rows_cell(s, row_first, n, j);
    return CellWhere{c, c >= 0 ? CELL_SIDE_A : -1};
}

// the id and the mask byte of a cell; `seq` = the ids of its sequence
BF_HD int32_t rows_cell_value(const RowsSpec &s, int64_t cell, const int32_t *seq, uint8_t *mask)
{
    *mask = cell == ROWS_CELL_PAD ? 0 : 1;
    return cell >= 0 ? seq[cell] : cell == ROWS_CELL_CLS ? s.cls_id : cell == ROWS_CELL_SEP ? s.sep_id : s.pad_id;
}

// row_first as the int32 the outputs hold: an index beyond INT32_MAX (one sequence of more than 2^31 ids) saturates (*saturated is set then)
BF_HD int32_t rows_first_i32(int64_t first, bool *saturated)
{
    *saturated = first > 0x7fffffff;
    return *saturated ? 0x7fffffff : (int32_t)first;
}

// the sequence of row r: the last q of [0, nseq) with row_off[q] <= r (every sequence has at least one row: the offsets rise strictly)
BF_HD int64_t rows_find_seq(const int64_t *row_off, int64_t nseq, int64_t r)
{
    int64_t lo = 0, hi = nseq - 1;
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if (row_off[mid] <= r) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// The rows stage's source, as bf_rowstage_body.h asks for one: items that are single ranges of one id array.  What a source supplies:
//   HAS_TYPE       whether a type plane exists
//   valid()        false = the arguments are refused (BF_E_ARG)
//   load(q)        item q: what the other calls need of it, `bad` = a range outside its array or decreasing offsets (read as empty)
//   count(it)      its rows, saturating at INT32_MAX
//   one_row()      one row per item is certain whatever the lengths: row r is item r and starts at the item's first id
//   first(it, k)   the first id of the item's row k
//   row(it, first) that row laid out once for all of its cells
//   cell(it, w, j) the id, the mask byte and the type byte of its cell j
//   where(it, w, j) which element of which id array that cell reads (CellWhere, `at` counted from the start of the array), or "not an id"
struct RowsSource {
    static constexpr bool HAS_TYPE = false;
    RowsSpec spec;
    const int32_t *ids; int64_t ids_len; const int64_t *id_off;      // sequence q = ids[id_off[q] .. id_off[q+1])

    struct Item { const int32_t *seq; int64_t n; bool bad; };
    struct Row { int64_t first; };

    BF_HD bool valid() const { return ids_len >= 0 && id_off && (ids_len == 0 || ids); }
    BF_HD Item load(int64_t q) const
    {
        Item it;
        const int64_t b = id_off[q];
        it.n = rows_seq_len(b, id_off[q + 1], ids_len, &it.bad);
        it.seq = ids + (it.bad ? 0 : b);
        return it;
    }
    BF_HD int32_t count(const Item &it, bool *saturated) const { return rows_count(spec, it.n, saturated); }
    BF_HD constexpr bool one_row() const { return false; }
    BF_HD int64_t first(const Item &, int64_t k) const { return k * spec.step; }
    BF_HD Row row(const Item &, int64_t first) const { return Row{first}; }
    BF_HD int32_t cell(const Item &it, const Row &w, int j, uint8_t *mask, uint8_t *type) const
    {
        *type = 0;
        return rows_cell_value(spec, rows_cell(spec, w.first, it.n, j), it.seq, mask);
    }
    BF_HD CellWhere where(const Item &it, const Row &w, int j) const
    {
        CellWhere c = rows_where(spec, w.first, it.n, j);
        c.at += it.seq - ids;
        return c;
    }
};

// ---- span cells (RowsSpanCellsBatchDevice): a byte span [a, z] (z inclusive) -> the cells of a row whose tokens hold its two ends.  S / E = the
// row's cells of a start plane and an end plane; only cells with S[j] >= 0 count.  start = max { j : S[j] <= a }, end = min { j : E[j] >= z };
// no order of the planes is assumed: every cell is looked at, the candidates are combined with max / min (k_rows_span: across lanes).
constexpr int ROWS_SPAN_NO_END = 0x7fffffff;

struct SpanAcc { int32_t start, end; };          // the best candidates so far: -1 / ROWS_SPAN_NO_END = none

BF_HD SpanAcc span_none() { return SpanAcc{-1, ROWS_SPAN_NO_END}; }

// what cell j contributes
BF_HD SpanAcc span_cell(int32_t s, int32_t e, int32_t a, int32_t z, int j)
{
    const bool in = s >= 0;
    return SpanAcc{in && s <= a ? j : -1, in && e >= z ? j : ROWS_SPAN_NO_END};
}

BF_HD SpanAcc span_combine(const SpanAcc &x, const SpanAcc &y) { return SpanAcc{x.start > y.start ? x.start : y.start, x.end < y.end ? x.end : y.end}; }

// the two cells of a row from what all of its cells contributed: none_cell twice unless the span is one (0 <= a <= z) and both ends were found
BF_HD void span_result(const SpanAcc &acc, int32_t a, int32_t z, int none_cell, int32_t *start_cell, int32_t *end_cell)
{
    const bool ok = a >= 0 && z >= a && acc.start >= 0 && acc.end != ROWS_SPAN_NO_END;
    *start_cell = ok ? acc.start : none_cell;
    *end_cell = ok ? acc.end : none_cell;
}

// lanes that share a row in k_rows_span: a wave (64), or the smallest power of two >= row_len where that is at most 32
BF_HD int span_group(int row_len)
{
    int g = 1;
    while (g < row_len && g < 64) g <<= 1;
    return g;
}

} // namespace bfa
