// bf_packedplanestest.cpp -- TEST-ONLY: the "where" lane code of the packed rows (blingfire_amd/csrc/bf_packed.h: packed_where, which packed_cell
// reads its ids by and k_packed_planes gathers by) compiled for the host and driven in the lane partition of k_packed_planes: the kernels of the
// base call in their order (widths, scan, next, the doubling rounds, the scan of the marks, the row starts), then every cell of every row below
// the capacity in lanes of `lane_cells` cells, the unit hint carried between a lane's cells.  With BF_PACKEDPLANESTEST_MAIN the file is a program
// of its own over exactly sized heap arrays (tests build it with -fsanitize=address,undefined).
#include <stddef.h>
#include <stdint.h>
#include <vector>
#include "../../blingfire_amd/csrc/bf_packed.h"

using namespace bfa;

extern "C" {

// IdsToPackedRowsPlanesBatchDevice, the planes alone: returns R, -1 for refused parameters.  src / fill / out: nplanes entries each (an out may be
// NULL: skipped); src[k] has ids_len elements and is read at id cells only.  rows_out (optional, [rows_cap * row_len]): the ids plane through
// packed_cell over `ids` (NULL: not taken), for a caller that wants both from one run.  *status: bit 0 rows dropped from a taken plane, bit 3 a bad range.
int64_t bft_packedplanes_batch(const int32_t *ids, int64_t ids_len, const int64_t *id_off, int64_t nseq, int row_len, int cls_id, int sep_id, int pad_id, int nplanes,
                               const int32_t *const *src, const int32_t *fill, int32_t *const *out, int32_t *rows_out, int64_t rows_cap, int lane_cells, int *status)
{
    PackedSpec sp;
    *status = 0;
    if (!packed_spec(row_len, cls_id, sep_id, pad_id, 0, &sp) || nseq < 0 || nseq > 0x7fffffff || ids_len < 0 || rows_cap < 0 || nplanes < 0 || nplanes > 4) return -1;
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
        for (int k = 0, rounds = packed_rounds(nseq); k < rounds; ++k)         // k_packed_double, one launch per round
            for (int64_t s = 0; s <= nseq; ++s) packed_double(jmp[k & 1].data(), jmp[(k & 1) ^ 1].data(), mark.data(), s);
    }
    for (int64_t q = 0; q < nseq; ++q) mark_off[(size_t)q + 1] = mark_off[(size_t)q] + mark[(size_t)q];
    const int64_t R = mark_off[(size_t)nseq];
    for (int64_t q = 0; q <= nseq; ++q)                                        // k_packed_rows
        if (q == nseq || mark[(size_t)q]) f[(size_t)mark_off[(size_t)q]] = (int32_t)q;
    bool any = false;
    for (int k = 0; k < nplanes; ++k) any = any || out[k];
    if (R > rows_cap && any) *status |= 1;                                     // lane 0 of k_packed_planes
    const int64_t nrows = R < rows_cap ? R : rows_cap;
    for (int64_t r = 0; r < nrows; ++r)                                        // k_packed_planes (and k_packed_fill for rows_out)
        for (int j0 = 0; j0 < row_len; j0 += lane_cells) {
            const int64_t s = f[(size_t)r], e = f[(size_t)r + 1];
            int64_t q = s, q_fill = s;
            for (int c = 0; c < lane_cells; ++c) {
                const int64_t w = packed_where(sp, W.data(), s, e, j0 + c, id_off, &q);
                const int64_t at = r * row_len + j0 + c;
                for (int k = 0; k < nplanes; ++k)
                    if (out[k]) out[k][at] = w != PACKED_NONE ? src[k][w] : fill[k];
                if (rows_out) rows_out[at] = packed_cell(sp, W.data(), s, e, j0 + c, ids, id_off, &q_fill).id;
            }
        }
    return R;
}

} // extern "C"

#ifdef BF_PACKEDPLANESTEST_MAIN
#include <cstdio>

// Exactly sized heap arrays (a read or a write past them is the sanitizer's to find).  Checked here: only what needs no second implementation --
// four cells per lane give what one cell per lane gives; a plane over the source {0, 1, 2, ...} names, in every cell where the ids plane over
// the ids {BASE, BASE + 1, ...} holds an id, that id's own index, and the fill everywhere else; rows at or past the capacity are not written.
namespace {

const int32_t BASE = 1 << 20, CANARY = -0x35014542;

int run_case(const std::vector<int64_t> &off, int64_t ids_len, int L, int cls, int sep)
{
    const int64_t nseq = (int64_t)off.size() - 1;
    std::vector<int32_t> ids((size_t)ids_len), src0((size_t)ids_len), src1((size_t)ids_len);
    for (int64_t i = 0; i < ids_len; ++i) { ids[(size_t)i] = BASE + (int32_t)i; src0[(size_t)i] = (int32_t)i; src1[(size_t)i] = (int32_t)(7 * i + 3); }
    const int32_t *src[2] = {src0.data(), src1.data()};
    const int32_t fill[2] = {-1, -9};
    int st = 0;
    int32_t *none[2] = {nullptr, nullptr};
    const int64_t R = bft_packedplanes_batch(ids.data(), ids_len, off.data(), nseq, L, cls, sep, 0, 2, src, fill, none, nullptr, 0, 1, &st);      // the size query
    if (R < 0 || (st & 1)) return 1;
    for (int64_t cap : {R, R > 1 ? R - 1 : R}) {             // (no capacity of 0 rows: an empty vector has no address to pass as a taken plane)
        const size_t n = (size_t)(cap * L);
        std::vector<int32_t> a0(n, CANARY), a1(n, CANARY), rows(n, CANARY), b0(n, CANARY), b1(n, CANARY);
        int32_t *oa[2] = {a0.data(), a1.data()}, *ob[2] = {b0.data(), b1.data()};
        int sa = 0, sb = 0;
        if (bft_packedplanes_batch(ids.data(), ids_len, off.data(), nseq, L, cls, sep, 0, 2, src, fill, oa, rows.data(), cap, 1, &sa) != R) return 1;
        if ((sa & 1) != (R > cap ? 1 : 0)) return 1;
        if (L % 4 == 0) {
            if (bft_packedplanes_batch(ids.data(), ids_len, off.data(), nseq, L, cls, sep, 0, 2, src, fill, ob, nullptr, cap, 4, &sb) != R || sb != sa) return 1;
            if (a0 != b0 || a1 != b1) return 1;
        }
        for (size_t c = 0; c < n; ++c) {
            const bool is_id = rows[c] >= BASE;
            if (a0[c] != (is_id ? rows[c] - BASE : -1) || a1[c] != (is_id ? 7 * (rows[c] - BASE) + 3 : -9)) return 1;
        }
        ob[0] = nullptr;                                       // a plane that is not taken, the other alone
        std::vector<int32_t> c1(n, CANARY);
        ob[1] = c1.data();
        if (bft_packedplanes_batch(ids.data(), ids_len, off.data(), nseq, L, cls, sep, 0, 2, src, fill, ob, nullptr, cap, 1, &sb) != R || c1 != a1) return 1;
    }
    return 0;
}

std::vector<int64_t> offsets(const std::vector<int64_t> &lens)
{
    std::vector<int64_t> off(lens.size() + 1, 0);
    for (size_t i = 0; i < lens.size(); ++i) off[i + 1] = off[i] + lens[i];
    return off;
}

} // namespace

int main()
{
    const int Ls[5] = {1, 4, 5, 8, 64};
    int64_t cases = 0;
    uint32_t x = 99991u;
    auto rnd = [&x]() { x = x * 1664525u + 1013904223u; return x >> 8; };
    auto run = [&](const std::vector<int64_t> &off, int64_t ids_len, int L, int cls, int sep, const char *what) {
        if (run_case(off, ids_len, L, cls, sep)) { fprintf(stderr, "FAILED: %s L %d cls %d sep %d\n", what, L, cls, sep); return 1; }
        ++cases;
        return 0;
    };
    for (int L : Ls) for (int cls : {101, -1}) for (int sep : {102, -1}) {
        const int body = L - (cls >= 0) - (sep >= 0);
        if (body < 1) continue;
        // the table's lengths in several orders, a truncated giant among them
        const std::vector<int64_t> t = {0, 1, body - 1, body, body + 1, 3 * body};
        std::vector<int64_t> lens(t);
        lens.insert(lens.end(), t.rbegin(), t.rend());
        for (size_t i = 0; i < t.size(); i += 2) lens.push_back(t[i]);
        for (size_t i = 1; i < t.size(); i += 2) lens.push_back(t[i]);
        lens.insert(lens.end(), {1, 1, 0, 0, 2000, 1});
        std::vector<int64_t> off = offsets(lens);
        if (run(off, off.back(), L, cls, sep, "table")) return 1;
        // random lengths with runs of empty sequences
        for (int seed = 0; seed < 3; ++seed) {
            lens.clear();
            for (int i = 0; i < 150; ++i) {
                if (rnd() % 20 == 0) for (int k = (int)(rnd() % 6); k >= 0; --k) lens.push_back(0);
                lens.push_back((int64_t)(rnd() % (uint32_t)(body + 3)) / (rnd() % 2 ? 4 : 1));
            }
            off = offsets(lens);
            if (run(off, off.back(), L, cls, sep, "mixed")) return 1;
        }
        // a long run of width-0 (or specials-only) units between two sequences
        lens.assign(3000, 0); lens.front() = 3; lens.back() = 2;
        off = offsets(lens);
        if (run(off, off.back(), L, cls, sep, "empty runs")) return 1;
        // bad ranges: decreasing, past ids_len, ids_len below the last offset, a negative first offset
        if (run({0, 5, 3, 12, 20}, 60, L, cls, sep, "decreasing")) return 1;
        if (run({0, 10, 70, 70, 80}, 60, L, cls, sep, "past ids_len")) return 1;
        if (run({0, 10, 20, 35, 60}, 30, L, cls, sep, "short ids_len")) return 1;
        if (run({-1, 4, 9}, 60, L, cls, sep, "negative")) return 1;
        if (run({0}, 0, L, cls, sep, "no sequences")) return 1;
    }
    for (int L : {4, 8, 64}) {                                 // exact fit without specials: widths that add up to L, and to L + 1
        std::vector<int64_t> lens;
        for (int a = 1; a < L - 1; ++a) { lens.push_back(a); lens.push_back(L - a); lens.push_back(a > 1 ? a : L); lens.push_back(a > 1 ? L - a + 1 : 1); }
        const std::vector<int64_t> off = offsets(lens);
        if (run(off, off.back(), L, -1, -1, "exact fit")) return 1;
    }
    printf("packedplanes ok: %lld cases\n", (long long)cases);
    return 0;
}
#endif
