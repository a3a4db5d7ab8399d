// bf_planestest.cpp -- TEST-ONLY: the "where" calls of the companion planes (blingfire_amd/csrc/bf_rows.h RowsSource::where, bf_pairs.h
// PairsSource::where) and the span predicate / combine (bf_rows.h span_*) compiled for the host.  The planes are driven the way k_rowstage_planes
// drives them (every cell of every row below the capacity on its own, the item loaded from the offsets again), the span cells in the lane
// partition of k_rows_span: G lanes per row, lane l takes cells l, l + G, ..., then a butterfly of xor exchanges inside the group.  With
// BF_PLANESTEST_MAIN the file is a program of its own over exactly sized heap arrays (tests build it with -fsanitize=address,undefined).
#include <stdint.h>
#include <stddef.h>
#include <vector>
#include "../../blingfire_amd/csrc/bf_pairs.h"

using namespace bfa;

namespace {

constexpr int MAX_PLANES = 4;

// Returns the row total (offsets complete); rows at or past rows_cap are not written.  src[side][k] may be NULL (the fill), out[k] too (skipped).
template <class S>
int64_t planes_stage(const S &src, int64_t nseq, int nplanes, const int32_t *const *src_a, const int32_t *const *src_b, const int32_t *fill, int32_t *const *out,
                     int64_t rows_cap, int64_t *row_off, int *status)
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
    bool any = false;
    for (int k = 0; k < nplanes; ++k) any = any || out[k];
    if (!any) return total;
    if (total > rows_cap) *status |= 1;
    const int64_t nrows = total < rows_cap ? total : rows_cap;
    for (int64_t r = 0; r < nrows; ++r) {
        const int64_t q = src.one_row() ? r : rows_find_seq(row_off, nseq, r);
        const typename S::Item it = src.load(q);
        const typename S::Row w = src.row(it, src.first(it, r - row_off[q]));
        for (int j = 0; j < row_len; ++j) {
            const CellWhere c = src.where(it, w, j);
            for (int k = 0; k < nplanes; ++k) {
                if (!out[k]) continue;
                const int32_t *from = c.side < 0 ? nullptr : c.side == CELL_SIDE_B ? (src_b ? src_b[k] : nullptr) : (src_a ? src_a[k] : nullptr);
                out[k][r * row_len + j] = from ? from[c.at] : fill[k];
            }
        }
    }
    return total;
}

} // namespace

extern "C" {

int64_t bft_rows_planes(const int32_t *ids, int64_t ids_len, const int64_t *id_off, int64_t nseq, int row_len, int cls_id, int sep_id, int stride, int max_rows,
                        int flags, int nplanes, const int32_t *const *src, const int32_t *fill, int32_t *const *out, int64_t rows_cap, int64_t *row_off, int *status)
{
    RowsSpec sp;
    *status = 0;
    if (!rows_spec(row_len, cls_id, sep_id, 0, stride, max_rows, flags, &sp) || nseq < 0 || ids_len < 0 || rows_cap < 0 || nplanes < 0 || nplanes > MAX_PLANES) return -1;
    return planes_stage(RowsSource{sp, ids, ids_len, id_off}, nseq, nplanes, src, nullptr, fill, out, rows_cap, row_off, status);
}

int64_t bft_pair_rows_planes(const int32_t *ids_a, int64_t len_a, const int64_t *off_a, const int32_t *ids_b, int64_t len_b, const int64_t *off_b, int64_t nseq,
                             int row_len, int cls_id, int sep_id, int mode, int max_a, int stride, int max_rows, int flags, int nplanes, const int32_t *const *src_a,
                             const int32_t *const *src_b, const int32_t *fill, int32_t *const *out, int64_t rows_cap, int64_t *row_off, int *status)
{
    PairsSpec sp;
    *status = 0;
    if (!pairs_spec(row_len, cls_id, sep_id, 0, mode, max_a, stride, max_rows, flags, &sp) || nseq < 0 || len_a < 0 || len_b < 0 || rows_cap < 0 || nplanes < 0 ||
        nplanes > MAX_PLANES) return -1;
    return planes_stage(PairsSource{sp, ids_a, ids_b, len_a, len_b, off_a, off_b}, nseq, nplanes, src_a, src_b, fill, out, rows_cap, row_off, status);
}

int bft_span_group(int row_len) { return span_group(row_len); }

// k_rows_span over nrows rows with `group` lanes per row (0 = span_group(row_len), the kernel's choice; any power of two up to 64 otherwise).
// Returns the status bits.
int bft_span_rows(const int32_t *S, const int32_t *E, int row_len, int64_t nrows, const int32_t *row_seq, int64_t nseq, const int32_t *span_first,
                  const int32_t *span_last, int none_cell, int32_t *start_cell, int32_t *end_cell, int group)
{
    const int G = group > 0 ? group : span_group(row_len);
    int status = 0;
    std::vector<SpanAcc> lane((size_t)G);
    for (int64_t r = 0; r < nrows; ++r) {
        const int64_t q = row_seq ? (int64_t)row_seq[r] : r;
        const bool known = q >= 0 && q < nseq;
        const int32_t a = known ? span_first[q] : -1, z = known ? span_last[q] : -1;
        for (int l = 0; l < G; ++l) {
            lane[(size_t)l] = span_none();
            if (known && a >= 0 && z >= a)
                for (int j = l; j < row_len; j += G) lane[(size_t)l] = span_combine(lane[(size_t)l], span_cell(S[r * row_len + j], E[r * row_len + j], a, z, j));
        }
        for (int m = G / 2; m > 0; m >>= 1) {
            std::vector<SpanAcc> next((size_t)G);
            for (int l = 0; l < G; ++l) next[(size_t)l] = span_combine(lane[(size_t)l], lane[(size_t)(l ^ m)]);
            lane.swap(next);
        }
        span_result(lane[0], a, z, none_cell, &start_cell[r], &end_cell[r]);
        if (!known) status |= 8;
    }
    return status;
}

} // extern "C"

#ifdef BF_PLANESTEST_MAIN
#include <cstdio>

// Rows and pair rows over exactly sized inputs, companion arrays and planes (a read or a write past them is the sanitizer's to find), then the span
// cells over the planes.  Checked here: only what needs no second implementation -- companion element i is 7 i + 1 on side A and -(7 i + 1) - 2 on side
// B with fill -1, so a plane holds the fill or values of one sign per side, rising by 7 along a row.
static int check_plane(const std::vector<int32_t> &pl, int64_t nrows, int L, bool pairs)
{
    for (int64_t r = 0; r < nrows; ++r) {
        int32_t last_a = 0, last_b = 0;
        for (int j = 0; j < L; ++j) {
            const int32_t v = pl[(size_t)(r * L + j)];
            if (v == -1) continue;
            if (v > 0) { if (v % 7 != 1 || (last_a && v != last_a + 7)) return 1; last_a = v; }
            else { if (!pairs || (-v - 2) % 7 != 1 || (last_b && v != last_b - 7)) return 1; last_b = v; }
        }
    }
    return 0;
}

static int run_rows(int L, int cls, int sep, int stride, int max_rows, int flags, int64_t cap_delta)
{
    RowsSpec sp;
    if (!rows_spec(L, cls, sep, 0, stride, max_rows, flags, &sp)) return 0;
    const int64_t lens[8] = {0, 1, sp.body - 1, sp.body, sp.body + 1, sp.body + sp.step, sp.body + sp.step + 1, (int64_t)3 * sp.body + 1};
    std::vector<int64_t> off(9, 0);
    for (int q = 0; q < 8; ++q) off[(size_t)q + 1] = off[(size_t)q] + lens[q];
    std::vector<int32_t> ids((size_t)off[8]), src((size_t)off[8]);
    for (size_t i = 0; i < ids.size(); ++i) { ids[i] = 1000 + (int32_t)i; src[i] = 7 * (int32_t)i + 1; }
    std::vector<int64_t> row_off(9);
    int status = 0;
    const int32_t *srcs[1] = {src.data()}; const int32_t fill[1] = {-1}; int32_t *none[1] = {nullptr};
    const int64_t total = bft_rows_planes(ids.data(), off[8], off.data(), 8, L, cls, sep, stride, max_rows, flags, 1, srcs, fill, none, 0, row_off.data(), &status);
    if (total < 8 || status != 0) return 1;
    const int64_t cap = total + cap_delta < 0 ? 0 : total + cap_delta, nrows = cap < total ? cap : total;
    std::vector<int32_t> pl((size_t)(cap * L));
    int32_t *outs[1] = {pl.data()};
    if (bft_rows_planes(ids.data(), off[8], off.data(), 8, L, cls, sep, stride, max_rows, flags, 1, srcs, fill, outs, cap, row_off.data(), &status) != total) return 1;
    if ((status & 1) != (total > cap ? 1 : 0) || check_plane(pl, nrows, L, false)) return 1;
    // the span cells over (plane, plane + 3) with one item per row
    std::vector<int32_t> E(pl), a((size_t)nrows), z((size_t)nrows), sc((size_t)nrows), ec((size_t)nrows);
    for (size_t i = 0; i < E.size(); ++i) if (E[i] >= 0) E[i] += 3;
    for (int64_t r = 0; r < nrows; ++r) { a[(size_t)r] = (int32_t)(7 * r % 50); z[(size_t)r] = a[(size_t)r] + (int32_t)(r % 20) - 1; }
    if (nrows > 0 && bft_span_rows(pl.data(), E.data(), L, nrows, nullptr, nrows, a.data(), z.data(), -100, sc.data(), ec.data(), 0) != 0) return 1;
    for (int64_t r = 0; r < nrows; ++r) {
        const int32_t s = sc[(size_t)r], e = ec[(size_t)r];
        if ((s == -100) != (e == -100)) return 1;
        if (s != -100 && (s < 0 || s >= L || e < 0 || e >= L || pl[(size_t)(r * L + s)] > a[(size_t)r] || E[(size_t)(r * L + e)] < z[(size_t)r])) return 1;
    }
    return 0;
}

static int run_pairs(int L, int cls, int sep, int mode, int max_a, int stride, int max_rows, int flags, int64_t cap_delta)
{
    PairsSpec sp;
    if (!pairs_spec(L, cls, sep, 0, mode, max_a, stride, max_rows, flags, &sp)) return 0;
    const int T = sp.room;
    const int64_t la[6] = {0, 1, max_a, max_a + 1, T, 3 * T}, lb[6] = {3 * T + 1, T, 0, T + 1, 1, 2 * T};
    std::vector<int64_t> off_a(7, 0), off_b(7, 0);
    for (int q = 0; q < 6; ++q) { off_a[(size_t)q + 1] = off_a[(size_t)q] + la[q]; off_b[(size_t)q + 1] = off_b[(size_t)q] + lb[q]; }
    std::vector<int32_t> ids_a((size_t)off_a[6]), ids_b((size_t)off_b[6]), src_a(ids_a.size()), src_b(ids_b.size());
    for (size_t i = 0; i < ids_a.size(); ++i) { ids_a[i] = 1000 + (int32_t)i; src_a[i] = 7 * (int32_t)i + 1; }
    for (size_t i = 0; i < ids_b.size(); ++i) { ids_b[i] = 500000 + (int32_t)i; src_b[i] = -(7 * (int32_t)i + 1) - 2; }
    std::vector<int64_t> row_off(7);
    int status = 0;
    const int32_t *sa[2] = {src_a.data(), nullptr}, *sb[2] = {src_b.data(), src_b.data()}; const int32_t fill[2] = {-1, -1}; int32_t *none[2] = {nullptr, nullptr};
    const int64_t total = bft_pair_rows_planes(ids_a.data(), off_a[6], off_a.data(), ids_b.data(), off_b[6], off_b.data(), 6, L, cls, sep, mode, max_a, stride, max_rows, flags, 2,
                                               sa, sb, fill, none, 0, row_off.data(), &status);
    if (total < 6 || status != 0) return 1;
    const int64_t cap = total + cap_delta < 0 ? 0 : total + cap_delta, nrows = cap < total ? cap : total;
    std::vector<int32_t> p0((size_t)(cap * L)), p1((size_t)(cap * L));
    int32_t *outs[2] = {p0.data(), p1.data()};
    if (bft_pair_rows_planes(ids_a.data(), off_a[6], off_a.data(), ids_b.data(), off_b[6], off_b.data(), 6, L, cls, sep, mode, max_a, stride, max_rows, flags, 2, sa, sb, fill,
                             outs, cap, row_off.data(), &status) != total) return 1;
    if ((status & 1) != (total > cap ? 1 : 0) || check_plane(p0, nrows, L, true) || check_plane(p1, nrows, L, true)) return 1;
    for (size_t i = 0; i < p1.size(); ++i) if (p1[i] > 0) return 1;          // (side A of plane 1 has no source: the fill)
    return 0;
}

int main()
{
    const int Ls[7] = {1, 4, 5, 8, 33, 64, 130};
    int64_t cases = 0;
    for (int L : Ls) for (int cls = -1; cls <= 101; cls += 102) for (int sepk = 0; sepk < 3; ++sepk) for (int left = 0; left <= 1; ++left) for (int64_t d = -1; d <= 1; ++d) {
        const int sep = sepk ? 102 : -1;
        for (int stride = 0; stride <= 1; ++stride) for (int max_rows = 0; max_rows <= 2; ++max_rows) {
            if (sepk < 2 && run_rows(L, cls, sep, stride, max_rows, left, d)) { fprintf(stderr, "FAILED: rows L %d cls %d sep %d stride %d max_rows %d left %d cap %+lld\n", L, cls, sep, stride, max_rows, left, (long long)d); return 1; }
            if (run_pairs(L, cls, sep, 0, 1, stride, max_rows, left | (sepk == 2 ? 2 : 0), d)) { fprintf(stderr, "FAILED: pairs L %d cls %d sep %d stride %d max_rows %d flags %d cap %+lld\n", L, cls, sep, stride, max_rows, left | (sepk == 2 ? 2 : 0), (long long)d); return 1; }
            cases += 2;
        }
        if (run_pairs(L, cls, sep, 1, 0, 0, 1, left | (sepk == 2 ? 2 : 0), d)) { fprintf(stderr, "FAILED: pairs mode 1 L %d cls %d sep %d cap %+lld\n", L, cls, sep, (long long)d); return 1; }
        ++cases;
    }
    printf("planes ok: %lld cases\n", (long long)cases);
    return 0;
}
#endif
