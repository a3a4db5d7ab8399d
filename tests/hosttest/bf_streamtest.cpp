// bf_streamtest.cpp -- TEST-ONLY: the lane code of the stream rows (blingfire_amd/csrc/bf_stream.h) compiled for the host and driven in the
// partition of the kernels of bf_kernels_stream.hip: the widths and their scan, the per-sequence outputs and the counts, then the fill tile by
// tile -- the three searches of the whole W as a wave makes them (a probe per lane and round, the ballot collected lane by lane), the tile's slice staged
// relative to the tile or, when it is longer than the staged capacity, searched in W itself, and every lane's cells through stream_cells.
// With BF_STREAMTEST_MAIN the file is a program of its own over exactly sized heap arrays (tests build it with -fsanitize=address,undefined).
#include <stddef.h>
#include <stdint.h>
#include <vector>
#include "../../blingfire_amd/csrc/bf_stream.h"

using namespace bfa;

namespace {

// wave_find_unit of the kernel file: the last q in [0, nseq) with W[q] <= t; *rounds counts the rounds of the longest search
int64_t wave_find_unit(const int64_t *W, int64_t nseq, int64_t t, int *rounds)
{
    int64_t lo = 0, hi = nseq;
    int n = 0;
    while (hi - lo > 1) {
        unsigned long long yes = 0;
        for (int lane = 0; lane < STREAM_PROBES; ++lane) {
            const int64_t at = stream_probe(lo, hi, lane);
            if (at >= 0 && W[at] <= t) yes |= 1ull << lane;
        }
        stream_narrow(&lo, &hi, yes);
        ++n;
    }
    if (n > *rounds) *rounds = n;
    return lo;
}

struct Outs { int32_t *rows, *seg, *pos, *labels, *first_seq, *first_pos; };

template <int C>
void store(const Outs &o, int64_t at, int64_t r, int j, const StreamCell *c, int32_t first_seq, int32_t first_pos)
{
    for (int k = 0; k < C; ++k) {
        if (o.rows) o.rows[at + k] = c[k].id;
        if (o.seg) o.seg[at + k] = c[k].seg;
        if (o.pos) o.pos[at + k] = c[k].pos;
        if (o.labels) o.labels[at + k] = c[k].label;
    }
    if (j == 0) {
        if (o.first_seq) o.first_seq[r] = first_seq;
        if (o.first_pos) o.first_pos[r] = first_pos;
    }
}

// k_stream_fill: every tile of the cell space in turn (a workgroup's tiles are independent of each other)
template <int C>
void fill(const StreamSpec &sp, const int32_t *ids, const int64_t *id_off, const int64_t *W, int64_t nseq, int64_t rows_cap, const Outs &o, int force_global,
          int64_t *paths, int *rounds)
{
    constexpr int TC = STREAM_TILE_LANES * C;
    const int L = sp.row_len;
    const int64_t T = W[nseq], R = stream_nrows(sp, T);
    const int64_t cells = (R < rows_cap ? R : rows_cap) * L;
    const bool want_label = o.labels != nullptr;
    std::vector<int32_t> s_wrel(STREAM_STAGE_UNITS + 1);
    std::vector<int64_t> s_delta(STREAM_STAGE_UNITS);
    for (int64_t t0 = 0; t0 < cells; t0 += TC) {
        int64_t qa = 0, qe = 0, f0 = 0, n = 0;
        bool staged = false;
        if (t0 < T) {
            const int64_t last = t0 + TC < T - 1 ? t0 + TC : T - 1;
            qa = wave_find_unit(W, nseq, t0, rounds);
            qe = wave_find_unit(W, nseq, last, rounds);
            f0 = wave_find_unit(W, nseq, t0 - t0 % L, rounds);
            n = qe - qa + 1;
            staged = n <= STREAM_STAGE_UNITS && !force_global;
            if (staged)
                for (int64_t i = 0; i <= n; ++i) {
                    s_wrel[(size_t)i] = stream_wrel(W[qa + i], t0);
                    if (i < n) s_delta[(size_t)i] = stream_delta(id_off[qa + i], W[qa + i], sp.lead);
                }
            ++paths[staged ? 0 : 1];
        }
        for (int lane = 0; lane < STREAM_TILE_LANES; ++lane) {
            const int64_t t = t0 + (int64_t)lane * C;
            if (t >= cells) break;
            const int64_t r = t / L;
            const int j = (int)(t - r * L);
            StreamCell c[C];
            int32_t first_seq = 0, first_pos = 0;
            if (t0 >= T) stream_cells<C>(sp, StreamGlobal{}, ids, T, t0, 0, t, j, want_label, c, &first_seq, &first_pos);
            else if (staged) stream_cells<C>(sp, StreamStaged{s_wrel.data(), s_delta.data(), t0, qa, (int)n}, ids, T, t0, f0, t, j, want_label, c, &first_seq, &first_pos);
            else stream_cells<C>(sp, StreamGlobal{W, id_off, qa, qe, sp.lead}, ids, T, t0, f0, t, j, want_label, c, &first_seq, &first_pos);
            store<C>(o, t, r, j, c, first_seq, first_pos);
        }
    }
}

} // namespace

extern "C" {

// the tile geometry: {lanes of a tile, cells a lane of the wide form takes, units a staged slice holds at most, probes of a search round}
void bft_stream_geometry(int *out)
{
    out[0] = STREAM_TILE_LANES; out[1] = STREAM_WIDE_CELLS; out[2] = STREAM_STAGE_UNITS; out[3] = STREAM_PROBES;
}

// IdsToStreamRowsBatchDevice: returns R, -1 for refused parameters.  Every output but nrows ({R, T}) may be NULL.  lane_cells: 1 or 4 (4 needs
// row_len % 4 == 0).  force_global: every tile takes the search of W itself.  info[3]: tiles that were staged, tiles that were not, the rounds
// of the longest search of the whole W.  *status: bit 0 rows dropped from a taken row output, bit 3 a bad range.
int64_t bft_stream_batch(const int32_t *ids, int64_t ids_len, const int64_t *id_off, int64_t nseq, int row_len, int bos_id, int eos_id, int pad_id, int ignore_label,
                         int flags, int32_t *rows, int32_t *seg, int32_t *pos, int32_t *labels, int32_t *first_seq, int32_t *first_pos, int64_t rows_cap,
                         int32_t *seq_row, int32_t *seq_col, int64_t *nrows, int lane_cells, int force_global, int64_t *info, int *status)
{
    StreamSpec sp;
    *status = 0;
    info[0] = info[1] = info[2] = 0;
    if (!stream_spec(row_len, bos_id, eos_id, pad_id, ignore_label, flags, &sp) || nseq < 0 || nseq > 0x7fffffff || ids_len < 0 || rows_cap < 0) return -1;
    if (stream_rows_bound(sp, ids_len, nseq) > 0x7fffffff) return -1;
    if ((lane_cells != 1 && lane_cells != STREAM_WIDE_CELLS) || (lane_cells == STREAM_WIDE_CELLS && row_len % 4 != 0)) return -1;
    std::vector<int64_t> W((size_t)nseq + 1, 0);
    for (int64_t q = 0; q < nseq; ++q) {                                       // k_stream_widths + scan
        bool bad;
        W[(size_t)q + 1] = W[(size_t)q] + stream_width(sp, id_off[q], id_off[q + 1], ids_len, &bad);
        if (bad) *status |= 8;
    }
    const int64_t T = W[(size_t)nseq], R = stream_nrows(sp, T);
    for (int64_t q = 0; q < nseq; ++q) {                                       // k_stream_seq
        int32_t row, col;
        stream_seq_cell(sp, W[(size_t)q], &row, &col);
        if (seq_row) seq_row[q] = row;
        if (seq_col) seq_col[q] = col;
    }
    nrows[0] = R; nrows[1] = T;
    const Outs o{rows, seg, pos, labels, first_seq, first_pos};
    const bool any = rows || seg || pos || labels || first_seq || first_pos;
    if (R > rows_cap && any) *status |= 1;
    int rounds = 0;
    if (any && rows_cap > 0) {
        if (lane_cells == 1) fill<1>(sp, ids, id_off, W.data(), nseq, rows_cap, o, force_global, info, &rounds);
        else fill<STREAM_WIDE_CELLS>(sp, ids, id_off, W.data(), nseq, rows_cap, o, force_global, info, &rounds);
    }
    info[2] = rounds;
    return R;
}

} // extern "C"

#ifdef BF_STREAMTEST_MAIN
#include <cstdio>

// Exactly sized heap arrays (a read or a write past them is the sanitizer's to find).  Checked here: only what needs no second implementation --
// four cells per lane give what one cell per lane gives; the search of W itself gives what the staged slice gives; rows at or past the
// capacity are not written; without specials and with good ranges the cells of the rows, in order, are the ids themselves; a label is the next
// cell's id (flags bit 2 off), the last one of the stream the ignored label; a search of the whole W takes at most six rounds.
namespace {

const int32_t BASE = 1 << 20, CANARY = -0x35014542, IGN = -100;

struct Run { int64_t R, T; std::vector<int32_t> a[6]; std::vector<int32_t> seq[2]; int status; int64_t info[3]; };

bool run_one(const std::vector<int32_t> &ids, int64_t ids_len, const std::vector<int64_t> &off, int L, int bos, int eos, int flags, int64_t cap, int lane_cells, int force, Run *out)
{
    const int64_t nseq = (int64_t)off.size() - 1;
    const size_t n = (size_t)(cap * L);
    for (int i = 0; i < 4; ++i) out->a[i].assign(n, CANARY);
    out->a[4].assign((size_t)cap, CANARY); out->a[5].assign((size_t)cap, CANARY);
    out->seq[0].assign((size_t)nseq, CANARY); out->seq[1].assign((size_t)nseq, CANARY);
    int64_t nrows[2] = {-1, -1};
    auto p = [](std::vector<int32_t> &v) { return v.empty() ? nullptr : v.data(); };
    out->R = bft_stream_batch(ids.empty() ? nullptr : ids.data(), ids_len, off.data(), nseq, L, bos, eos, 0, IGN, flags, p(out->a[0]), p(out->a[1]), p(out->a[2]), p(out->a[3]),
                              p(out->a[4]), p(out->a[5]), cap, p(out->seq[0]), p(out->seq[1]), nrows, lane_cells, force, out->info, &out->status);
    out->T = nrows[1];
    return out->R >= 0 && nrows[0] == out->R;
}

int run_case(const std::vector<int64_t> &off, int64_t ids_len, int L, int bos, int eos, int flags, bool good)
{
    const int64_t real = ids_len > 0 ? ids_len : 0;
    std::vector<int32_t> ids((size_t)real);
    for (int64_t i = 0; i < real; ++i) ids[(size_t)i] = BASE + (int32_t)i;
    Run q;
    if (!run_one(ids, ids_len, off, L, bos, eos, flags, 0, 1, 0, &q) || (q.status & 1)) return 1;      // the size query: no row output has an address
    const int64_t R = q.R, T = q.T;
    for (int64_t cap : {R, R > 1 ? R - 1 : R}) {
        Run a, b;
        if (!run_one(ids, ids_len, off, L, bos, eos, flags, cap, 1, 0, &a) || a.R != R || a.T != T) return 2;
        if (cap > 0 && (a.status & 1) != (R > cap ? 1 : 0)) return 3;
        if (a.info[2] > 6) return 4;
        if (!run_one(ids, ids_len, off, L, bos, eos, flags, cap, 1, 1, &b)) return 5;
        for (int i = 0; i < 6; ++i) if (a.a[i] != b.a[i]) return 6;
        if (L % 4 == 0) {
            for (int force = 0; force < 2; ++force) {
                if (!run_one(ids, ids_len, off, L, bos, eos, flags, cap, 4, force, &b) || b.status != a.status) return 7;
                for (int i = 0; i < 6; ++i) if (a.a[i] != b.a[i]) return 8;
            }
        }
        const int64_t cells = cap * L;
        for (int64_t t = 0; t < cells; ++t) {
            const int32_t id = a.a[0][(size_t)t], lab = a.a[3][(size_t)t];
            if (id == CANARY || lab == CANARY || a.a[1][(size_t)t] == CANARY || a.a[2][(size_t)t] == CANARY) return 9;
            if (t >= T && (id != 0 || lab != IGN || a.a[1][(size_t)t] != 0)) return 10;
            if (good && bos < 0 && eos < 0 && t < T && id != BASE + (int32_t)(off[0] + t)) return 11;
            if (!(flags & STREAM_LABELS_WITHIN) && t + 1 < cells && t + 1 < T && lab != a.a[0][(size_t)t + 1]) return 12;
            if (t + 1 == T && lab != IGN) return 13;
        }
        for (int64_t r = 0; r < cap; ++r)
            if (a.a[4][(size_t)r] == CANARY || a.a[1][(size_t)(r * L)] != 1) return 14;
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
    const int Ls[6] = {1, 2, 4, 5, 8, 64};
    int64_t cases = 0;
    uint32_t x = 99991u;
    auto rnd = [&x]() { x = x * 1664525u + 1013904223u; return x >> 8; };
    auto run = [&](const std::vector<int64_t> &off, int64_t ids_len, int L, int bos, int eos, int flags, bool good, const char *what) {
        const int rc = run_case(off, ids_len, L, bos, eos, flags, good);
        if (rc) { fprintf(stderr, "FAILED (%d): %s L %d bos %d eos %d flags %d\n", rc, what, L, bos, eos, flags); return 1; }
        ++cases;
        return 0;
    };
    const int TCW = STREAM_TILE_LANES * STREAM_WIDE_CELLS, SU = STREAM_STAGE_UNITS;
    for (int L : Ls) for (int bos : {1, -1}) for (int eos : {2, -1}) for (int flags = 0; flags < 8; ++flags) {
        std::vector<int64_t> lens = {0, 1, L - 1, L, L + 1, 3 * L, 0, 0, 2, 7 * L + 3, 1, 1, 0};
        std::vector<int64_t> off = offsets(lens);
        if (run(off, off.back(), L, bos, eos, flags, true, "table")) return 1;
        lens.clear();
        for (int i = 0; i < 120; ++i) {                       // random lengths with runs of empty sequences
            if (rnd() % 20 == 0) for (int k = (int)(rnd() % 6); k >= 0; --k) lens.push_back(0);
            lens.push_back((int64_t)(rnd() % (uint32_t)(3 * L + 3)) / (rnd() % 2 ? 4 : 1));
        }
        off = offsets(lens);
        if (run(off, off.back(), L, bos, eos, flags, true, "mixed")) return 1;
        if (flags != 0 && flags != 7) continue;
        // bad ranges: decreasing, past ids_len, ids_len below the last offset, a negative first offset; no sequences; units of width 0 only
        if (run({0, 5, 3, 12, 20}, 60, L, bos, eos, flags, false, "decreasing")) return 1;
        if (run({0, 10, 70, 70, 80}, 60, L, bos, eos, flags, false, "past ids_len")) return 1;
        if (run({0, 10, 20, 35, 60}, 30, L, bos, eos, flags, false, "short ids_len")) return 1;
        if (run({-1, 4, 9}, 60, L, bos, eos, flags, false, "negative")) return 1;
        if (run({0}, 0, L, bos, eos, flags, true, "no sequences")) return 1;
        if (run({0, 0, 0, 0}, 0, L, bos, eos, flags, true, "empty sequences")) return 1;
    }
    for (int L : {4, 5, 8, 2 * TCW + 4}) for (int sp = 0; sp < 2; ++sp) {          // the tile: the staged capacity, a tile's edge, long runs of width 0
        const int bos = sp ? 1 : -1, eos = sp ? 2 : -1;
        const int tc = L % 4 == 0 ? TCW : STREAM_TILE_LANES;
        for (int d = -1; d <= 1; ++d) {
            std::vector<int64_t> lens = {tc + 10};
            lens.insert(lens.end(), (size_t)(SU + d - 5), 0);
            lens.insert(lens.end(), {1, 1, 2, tc});
            std::vector<int64_t> off = offsets(lens);
            if (run(off, off.back(), L, bos, eos, 0, true, "capacity")) return 1;
            lens = {tc + d, 7, tc - 7 - d, 9};
            off = offsets(lens);
            if (run(off, off.back(), L, bos, eos, 4, true, "edge")) return 1;
        }
        std::vector<int64_t> lens(3000, 0);
        lens.front() = 3; lens.back() = 2; lens[1500] = 3 * tc + 11;
        std::vector<int64_t> off = offsets(lens);
        if (run(off, off.back(), L, bos, eos, 2, true, "empty runs")) return 1;
    }
    printf("stream ok: %lld cases\n", (long long)cases);
    return 0;
}
#endif
