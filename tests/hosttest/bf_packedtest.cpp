// bf_packedtest.cpp -- TEST-ONLY: the lane code of IdsToPackedRowsBatch (blingfire_amd/csrc/bf_packed.h) compiled for the host and driven
// sequentially over the lane ranges of the kernels of bf_kernels_packed.hip, and nothing more: a width per sequence, a scan, next per sequence,
// the doubling rounds over the whole array (double-buffered, as many as packed_rounds says), a scan of the marks, the row of every sequence,
// then every cell of every row below the capacity in lanes of `lane_cells` cells.
#include <stddef.h>
#include <stdint.h>
#include <vector>
#include "../../blingfire_amd/csrc/bf_packed.h"

using namespace bfa;

extern "C" {

// IdsToPackedRowsBatchDevice: returns R, -1 for refused parameters.  *status: bit 0 rows dropped, bit 3 a sequence outside [0, ids_len].  Every
// output may be NULL; row_first has rows_cap + 1 entries.  lane_cells: 4 (row_len % 4 == 0 only) or 1.  next_out (optional, [nseq + 1]): next.
int64_t bft_packed_batch(const int32_t *ids, int64_t ids_len, const int64_t *id_off, int64_t nseq, int row_len, int cls_id, int sep_id, int pad_id, int flags,
                         int32_t *rows, int32_t *seg, int32_t *pos, int32_t *row_first, int64_t rows_cap, int32_t *seq_row, int32_t *seq_col, int lane_cells,
                         int32_t *next_out, int *status)
{
    PackedSpec sp;
    *status = 0;
    if (!packed_spec(row_len, cls_id, sep_id, pad_id, flags, &sp) || nseq < 0 || nseq > 0x7fffffff || ids_len < 0 || rows_cap < 0) return -1;
    if ((lane_cells != 1 && lane_cells != 4) || (lane_cells == 4 && row_len % 4 != 0)) return -1;
    const size_t n1 = (size_t)nseq + 1;
    std::vector<int64_t> W(n1, 0), mark_off(n1, 0);
    std::vector<int32_t> jmp[2] = {std::vector<int32_t>(n1), std::vector<int32_t>(n1)}, mark(n1, 0), f(n1, 0);
    for (int64_t q = 0; q < nseq; ++q) {                                       // k_packed_widths + scan
        bool bad;
        const int64_t n = rows_seq_len(id_off[q], id_off[q + 1], ids_len, &bad);
        if (bad) *status |= 8;
        W[(size_t)q + 1] = W[(size_t)q] + packed_width(sp, n);
    }
    if (nseq > 0) {
        for (int64_t s = 0; s <= nseq; ++s) {                                  // k_packed_next
            jmp[0][(size_t)s] = s < nseq ? packed_next(W.data(), nseq, s, row_len) : (int32_t)nseq;
            mark[(size_t)s] = s == 0 ? 1 : 0;
        }
        if (next_out) for (int64_t s = 0; s <= nseq; ++s) next_out[s] = jmp[0][(size_t)s];
        for (int k = 0, rounds = packed_rounds(nseq); k < rounds; ++k)         // k_packed_double, one launch per round
            for (int64_t s = 0; s <= nseq; ++s) packed_double(jmp[k & 1].data(), jmp[(k & 1) ^ 1].data(), mark.data(), s);
    } else if (next_out) next_out[0] = 0;
    for (int64_t q = 0; q < nseq; ++q) mark_off[(size_t)q + 1] = mark_off[(size_t)q] + mark[(size_t)q];      // scan of mark[0 .. nseq)
    const int64_t R = mark_off[(size_t)nseq];
    for (int64_t q = 0; q <= nseq; ++q) {                                      // k_packed_rows
        const int64_t r = mark_off[(size_t)q];
        const int m = q < nseq ? mark[(size_t)q] : 1;
        if (m) {
            f[(size_t)r] = (int32_t)q;
            if (row_first && r <= rows_cap) row_first[r] = (int32_t)q;
        }
        if (q < nseq && seq_row) seq_row[q] = (int32_t)(r + m - 1);
    }
    if (R > rows_cap && (rows || seg || pos || row_first)) *status |= 1;
    if (seq_col)                                                               // k_packed_cols
        for (int64_t q = 0; q < nseq; ++q) seq_col[q] = (int32_t)(W[(size_t)q] - W[(size_t)f[(size_t)(mark_off[(size_t)q] + mark[(size_t)q] - 1)]]);
    if (!rows && !seg && !pos) return R;
    const int64_t nrows = R < rows_cap ? R : rows_cap;
    for (int64_t r = 0; r < nrows; ++r)                                        // k_packed_fill
        for (int j0 = 0; j0 < row_len; j0 += lane_cells) {
            const int64_t s = f[(size_t)r], e = f[(size_t)r + 1];
            int64_t q = s;
            for (int k = 0; k < lane_cells; ++k) {
                const PackedCell c = packed_cell(sp, W.data(), s, e, j0 + k, ids, id_off, &q);
                const int64_t at = r * row_len + j0 + k;
                if (rows) rows[at] = c.id;
                if (seg) seg[at] = c.seg;
                if (pos) pos[at] = c.pos;
            }
        }
    return R;
}

} // extern "C"
