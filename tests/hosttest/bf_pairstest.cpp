// bf_pairstest.cpp -- TEST-ONLY: the pair-row logic of IdsToPairRowsBatch (blingfire_amd/csrc/bf_pairs.h) compiled for the host and driven
// sequentially, the way the kernels drive it on the device (bf_rowstagetest.h).  With BF_PAIRSTEST_MAIN the file is a program of its own that
// runs the parameter table over exactly sized heap arrays (tests build it with -fsanitize=address,undefined).
#include <stdint.h>
#include <vector>
#include "bf_rowstagetest.h"
#include "../../blingfire_amd/csrc/bf_pairs.h"

using namespace bfa;

extern "C" {

// IdsToPairRowsBatchDevice: returns the row total (offsets complete), -1 for refused parameters; rows at or past rows_cap are not written.
// *status: bit 0 rows dropped / a saturated count or index, bit 3 a range outside [0, len].  Each of the five outputs may be NULL.
int64_t bft_pair_rows_batch(const int32_t *ids_a, int64_t len_a, const int64_t *off_a, const int32_t *ids_b, int64_t len_b, const int64_t *off_b, int64_t nseq,
                            int row_len, int cls_id, int sep_id, int pad_id, int mode, int max_a, int stride, int max_rows, int flags, int32_t *rows,
                            uint8_t *mask, uint8_t *type, int32_t *row_seq, int32_t *row_first, int64_t rows_cap, int64_t *row_off, int *status)
{
    PairsSpec sp;
    *status = 0;
    if (!pairs_spec(row_len, cls_id, sep_id, pad_id, mode, max_a, stride, max_rows, flags, &sp) || nseq < 0 || len_a < 0 || len_b < 0 || rows_cap < 0) return -1;
    return bft_rowstage(PairsSource{sp, ids_a, ids_b, len_a, len_b, off_a, off_b}, nseq, rows, mask, type, row_seq, row_first, rows_cap, row_off, status);
}

} // extern "C"

#ifdef BF_PAIRSTEST_MAIN
#include <cstdio>

// One run of the table's pair lengths under one parameter set; the inputs and the outputs are exactly sized, so a read or a write past them
// is the sanitizer's to find.  Checked here: only what needs no second implementation (A ids 1000.., B ids 500000..: the A ids of a row are
// the first ids of its A with type 0, its B ids consecutive ids of its B from row_first on with type 1, the mask counts them and the specials).
static int run_case(int L, int cls, int sep, int mode, int max_a, int stride, int max_rows, int flags, int64_t cap_delta)
{
    PairsSpec sp;
    if (!pairs_spec(L, cls, sep, 0, mode, max_a, stride, max_rows, flags, &sp)) return 0;
    const int T = sp.room, h0 = T / 2, h1 = (T + 1) / 2;
    std::vector<int64_t> la, lb;
    if (mode == 0) {
        const int64_t nas[5] = {0, 1, max_a - 1, max_a, max_a + 1};
        for (int64_t na : nas) {
            if (na < 0) continue;
            const PairGeom g = pairs_geom(sp, na, 0);
            const int64_t nbs[8] = {0, 1, g.body_b - 1, g.body_b, g.body_b + 1, g.body_b + g.step, g.body_b + g.step + 1, (int64_t)3 * g.body_b + 1};
            for (int64_t nb : nbs) { la.push_back(na); lb.push_back(nb); }
        }
    } else {
        const int64_t ns[8] = {0, 1, h0, h1, h1 + 1, T, T + 1, (int64_t)3 * T};
        for (int64_t na : ns) for (int64_t nb : ns) { la.push_back(na); lb.push_back(nb); }
    }
    const int64_t n = (int64_t)la.size();
    std::vector<int64_t> off_a((size_t)n + 1, 0), off_b((size_t)n + 1, 0);
    for (int64_t q = 0; q < n; ++q) { off_a[(size_t)q + 1] = off_a[(size_t)q] + la[(size_t)q]; off_b[(size_t)q + 1] = off_b[(size_t)q] + lb[(size_t)q]; }
    std::vector<int32_t> ids_a((size_t)off_a[(size_t)n]), ids_b((size_t)off_b[(size_t)n]);
    for (size_t i = 0; i < ids_a.size(); ++i) ids_a[i] = 1000 + (int32_t)i;
    for (size_t i = 0; i < ids_b.size(); ++i) ids_b[i] = 500000 + (int32_t)i;
    std::vector<int64_t> row_off((size_t)n + 1);
    int status = 0;
    const int64_t total = bft_pair_rows_batch(ids_a.data(), off_a[(size_t)n], off_a.data(), ids_b.data(), off_b[(size_t)n], off_b.data(), n, L, cls, sep, 0, mode, max_a, stride,
                                              max_rows, flags, nullptr, nullptr, nullptr, nullptr, nullptr, 0, row_off.data(), &status);
    if (total < n || status != 0) { fprintf(stderr, "size query: total %lld status %d\n", (long long)total, status); return 1; }
    const int64_t cap = total + cap_delta < 0 ? 0 : total + cap_delta, nrows = cap < total ? cap : total;
    std::vector<int32_t> rows((size_t)(cap * L)), seq((size_t)cap), first((size_t)cap);
    std::vector<uint8_t> mask((size_t)(cap * L)), type((size_t)(cap * L));
    if (bft_pair_rows_batch(ids_a.data(), off_a[(size_t)n], off_a.data(), ids_b.data(), off_b[(size_t)n], off_b.data(), n, L, cls, sep, 0, mode, max_a, stride, max_rows, flags,
                            rows.data(), mask.data(), type.data(), seq.data(), first.data(), cap, row_off.data(), &status) != total) return 1;
    if ((status & 1) != (total > cap ? 1 : 0)) { fprintf(stderr, "status %d at cap %lld of %lld\n", status, (long long)cap, (long long)total); return 1; }
    for (int64_t r = 0; r < nrows; ++r) {
        const int64_t q = seq[(size_t)r];
        if (q < 0 || q >= n || r < row_off[(size_t)q] || r >= row_off[(size_t)q + 1]) { fprintf(stderr, "row %lld: pair %lld\n", (long long)r, (long long)q); return 1; }
        int ones = 0, ones_t = 0; int64_t next_a = off_a[(size_t)q], next_b = off_b[(size_t)q] + first[(size_t)r];
        for (int j = 0; j < L; ++j) {
            const int32_t v = rows[(size_t)(r * L + j)];
            const int m = mask[(size_t)(r * L + j)], t = type[(size_t)(r * L + j)];
            ones += m; ones_t += t;
            if (v >= 500000) { if (v != 500000 + next_b || !m || t != 1) { fprintf(stderr, "row %lld cell %d: B id %d\n", (long long)r, j, v); return 1; } ++next_b; }
            else if (v >= 1000) { if (v != 1000 + next_a || !m || t != 0) { fprintf(stderr, "row %lld cell %d: A id %d\n", (long long)r, j, v); return 1; } ++next_a; }
        }
        const int64_t ka = next_a - off_a[(size_t)q], kb = next_b - off_b[(size_t)q] - first[(size_t)r];
        if (ones != ka + kb + sp.lead + sp.mid + sp.trail || ones_t != kb + sp.trail || ka + kb > T || ka > la[(size_t)q] || first[(size_t)r] + kb > lb[(size_t)q] ||
            (mode == 1 && ka + kb < T && (ka < la[(size_t)q] || kb < lb[(size_t)q]))) {      // (longest first drops nothing while there is room)
            fprintf(stderr, "row %lld: %d real cells, %lld + %lld ids\n", (long long)r, ones, (long long)ka, (long long)kb); return 1;
        }
    }
    return 0;
}

int main()
{
    const int Ls[6] = {4, 5, 8, 63, 64, 130};
    int64_t cases = 0;
    for (int L : Ls) for (int cls = -1; cls <= 101; cls += 102) for (int sepk = 0; sepk < 3; ++sepk) for (int left = 0; left <= 1; ++left) {
        const int sep = sepk ? 102 : -1, flags = left | (sepk == 2 ? 2 : 0);
        const int T = L - (cls >= 0) - (sepk ? sepk + 1 : 0);
        if (T < 1) continue;
        for (int64_t d = -1; d <= 1; ++d) {
            if (run_case(L, cls, sep, 1, 0, 0, 1, flags, d)) { fprintf(stderr, "FAILED: mode 1 L %d cls %d sep %d flags %d cap %+lld\n", L, cls, sep, flags, (long long)d); return 1; }
            ++cases;
        }
        const int max_as[3] = {0, 1, T - 1};
        for (int ai = 0; ai < 3; ++ai) {
            const int max_a = max_as[ai];
            if (max_a > T - 1 || (ai > 0 && max_a == max_as[ai - 1])) continue;
            const int strides[3] = {0, 1, T - max_a - 1};
            for (int si = 0; si < 3; ++si) {
                if (strides[si] >= T - max_a || (si > 0 && strides[si] == strides[si - 1])) continue;
                for (int max_rows = 0; max_rows <= 3; ++max_rows) for (int64_t d = -1; d <= 1; ++d) {
                    if (run_case(L, cls, sep, 0, max_a, strides[si], max_rows, flags, d)) {
                        fprintf(stderr, "FAILED: mode 0 L %d cls %d sep %d max_a %d stride %d max_rows %d flags %d cap %+lld\n", L, cls, sep, max_a, strides[si], max_rows, flags, (long long)d);
                        return 1;
                    }
                    ++cases;
                }
            }
        }
    }
    printf("pairs ok: %lld cases\n", (long long)cases);
    return 0;
}
#endif
