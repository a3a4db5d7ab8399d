// bf_rowstest.cpp -- TEST-ONLY: the row logic of IdsToRowsBatch (blingfire_amd/csrc/bf_rows.h) compiled for the host and driven sequentially,
// the way the kernels drive it on the device (bf_rowstagetest.h).  With BF_ROWSTEST_MAIN the file is a program of its own that runs the parameter
// table over exactly sized heap arrays (tests build it with -fsanitize=address,undefined).
#include <stdint.h>
#include <vector>
#include "bf_rowstagetest.h"

using namespace bfa;

extern "C" {

// IdsToRowsBatchDevice: returns the row total (offsets complete), -1 for refused parameters; rows at or past rows_cap are not written.
// *status: bit 0 rows dropped / a saturated count, bit 3 a sequence outside [0, ids_len].  Each of the four outputs may be NULL.
int64_t bft_rows_batch(const int32_t *ids, int64_t ids_len, const int64_t *id_off, int64_t nseq, int row_len, int cls_id, int sep_id, int pad_id,
                         int stride, int max_rows, int flags, int32_t *rows, uint8_t *mask, int32_t *row_seq, int32_t *row_first, int64_t rows_cap,
                         int64_t *row_off, int *status)
{
    RowsSpec sp;
    *status = 0;
    if (!rows_spec(row_len, cls_id, sep_id, pad_id, stride, max_rows, flags, &sp) || nseq < 0 || ids_len < 0 || rows_cap < 0) return -1;
    return bft_rowstage(RowsSource{sp, ids, ids_len, id_off}, nseq, rows, mask, nullptr, row_seq, row_first, rows_cap, row_off, status);
}

} // extern "C"

#ifdef BF_ROWSTEST_MAIN
#include <cstdio>

// One run of the table's sequence lengths under one parameter set; the outputs have exactly total (or cap) rows, so a write past them is
// the sanitizer's to find.  Checked here: only what needs no second implementation (the mask counts the ids and specials of every
// sequence once per overlap-free window start, the ids of a row are consecutive ids of its sequence).
static int run_case(int L, int cls, int sep, int stride, int max_rows, int flags, int64_t cap_delta)
{
    RowsSpec sp;
    if (!rows_spec(L, cls, sep, 0, stride, max_rows, flags, &sp)) return 0;
    const int body = sp.body, step = sp.step;
    const int64_t lens[8] = {0, 1, body - 1, body, body + 1, body + step, body + step + 1, (int64_t)3 * body + 1};
    std::vector<int64_t> off(9, 0);
    for (int q = 0; q < 8; ++q) off[(size_t)q + 1] = off[(size_t)q] + lens[q];
    std::vector<int32_t> ids((size_t)off[8]);
    for (size_t i = 0; i < ids.size(); ++i) ids[i] = 1000 + (int32_t)i;
    std::vector<int64_t> row_off(9);
    int status = 0;
    const int64_t total = bft_rows_batch(ids.data(), off[8], off.data(), 8, L, cls, sep, 0, stride, max_rows, flags, nullptr, nullptr, nullptr, nullptr, 0, row_off.data(), &status);
    if (total < 8 || status != 0) { fprintf(stderr, "size query: total %lld status %d\n", (long long)total, status); return 1; }
    const int64_t cap = total + cap_delta < 0 ? 0 : total + cap_delta, nrows = cap < total ? cap : total;
    std::vector<int32_t> rows((size_t)(cap * L)), seq((size_t)cap), first((size_t)cap);
    std::vector<uint8_t> mask((size_t)(cap * L));
    if (bft_rows_batch(ids.data(), off[8], off.data(), 8, L, cls, sep, 0, stride, max_rows, flags, rows.data(), mask.data(), seq.data(), first.data(), cap, row_off.data(), &status) != total) return 1;
    if ((status & 1) != (total > cap ? 1 : 0)) { fprintf(stderr, "status %d at cap %lld of %lld\n", status, (long long)cap, (long long)total); return 1; }
    for (int64_t r = 0; r < nrows; ++r) {
        const int q = seq[(size_t)r];
        if (q < 0 || q >= 8 || r < row_off[(size_t)q] || r >= row_off[(size_t)q + 1]) { fprintf(stderr, "row %lld: sequence %d\n", (long long)r, q); return 1; }
        int64_t k = lens[q] - first[(size_t)r]; if (k > body) k = body; if (k < 0) k = 0;
        int ones = 0; int64_t next = off[(size_t)q] + first[(size_t)r];
        for (int j = 0; j < L; ++j) {
            const int32_t v = rows[(size_t)(r * L + j)];
            ones += mask[(size_t)(r * L + j)];
            if (v >= 1000) { if (v != 1000 + next || !mask[(size_t)(r * L + j)]) { fprintf(stderr, "row %lld cell %d: id %d\n", (long long)r, j, v); return 1; } ++next; }
        }
        if (ones != k + sp.lead + sp.trail || next != off[(size_t)q] + first[(size_t)r] + k) { fprintf(stderr, "row %lld: %d real cells, %lld ids\n", (long long)r, ones, (long long)k); return 1; }
    }
    return 0;
}

int main()
{
    const int Ls[9] = {1, 2, 3, 4, 5, 8, 63, 64, 130};
    int64_t cases = 0;
    for (int L : Ls) for (int cls = -1; cls <= 101; cls += 102) for (int sep = -1; sep <= 102; sep += 103) {
        const int body = L - (cls >= 0) - (sep >= 0);
        if (body < 1) continue;
        const int strides[3] = {0, 1, body - 1};
        for (int si = 0; si < 3; ++si) {
            if (strides[si] >= body || (si > 0 && strides[si] == strides[si - 1])) continue;
            for (int max_rows = 0; max_rows <= 3; ++max_rows) for (int flags = 0; flags <= 1; ++flags) for (int64_t d = -1; d <= 1; ++d) {
                if (run_case(L, cls, sep, strides[si], max_rows, flags, d)) { fprintf(stderr, "FAILED: L %d cls %d sep %d stride %d max_rows %d flags %d cap %+lld\n", L, cls, sep, strides[si], max_rows, flags, (long long)d); return 1; }
                ++cases;
            }
        }
    }
    printf("rows ok: %lld cases\n", (long long)cases);
    return 0;
}
#endif
