// bf_rowstagetest.h -- TEST-ONLY: the row stage (blingfire_amd/csrc/bf_rowstage_body.h) restated for the host over a source S (bf_rows.h RowsSource,
// bf_pairs.h PairsSource) and driven sequentially, the way the kernels drive it on the device: a count per item, a scan, the item and first id
// of every row below the capacity, then every cell of those rows on its own, with the item loaded from the offsets again.
#pragma once
#include <stdint.h>
#include "../../blingfire_amd/csrc/bf_rows.h"

// Returns the row total (offsets complete); rows at or past rows_cap are not written.  *status: bit 0 rows dropped / a saturated count or
// index, bit 3 a range outside its array.  Each output may be NULL (type: always, where S has none).
template <class S>
int64_t bft_rowstage(const S &src, int64_t nseq, int32_t *rows, uint8_t *mask, uint8_t *type, int32_t *row_seq, int32_t *row_first, int64_t rows_cap,
                     int64_t *row_off, int *status)
{
    const int row_len = src.spec.row_len;
    row_off[0] = 0;
    for (int64_t q = 0; q < nseq; ++q) {
        const typename S::Item it = src.load(q);
        bool sat;
        row_off[q + 1] = row_off[q] + src.count(it, &sat);
        if (it.bad) *status |= 8;
        if (sat) *status |= 1;
    }
    const int64_t total = row_off[nseq];
    if (!rows && !mask && !type && !row_seq && !row_first) return total;
    if (total > rows_cap) *status |= 1;
    const int64_t nrows = total < rows_cap ? total : rows_cap;
    for (int64_t r = 0; r < nrows; ++r) {
        const int64_t q = src.one_row() ? r : bfa::rows_find_seq(row_off, nseq, r);
        const typename S::Item it = src.load(q);
        const int64_t first = src.first(it, r - row_off[q]);
        if (row_seq) row_seq[r] = (int32_t)q;
        bool fsat;
        const int32_t first32 = bfa::rows_first_i32(first, &fsat);
        if (row_first) row_first[r] = first32;
        if (fsat) *status |= 1;
        const typename S::Row w = src.row(it, first);
        for (int j = 0; j < row_len && (rows || mask || type); ++j) {
            uint8_t m, t;
            const int32_t v = src.cell(it, w, j, &m, &t);
            if (rows) rows[r * row_len + j] = v;
            if (mask) mask[r * row_len + j] = m;
            if (type) type[r * row_len + j] = t;
        }
    }
    return total;
}
