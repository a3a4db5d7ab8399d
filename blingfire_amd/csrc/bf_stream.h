// bf_stream.h -- stream rows from ragged ids: every sequence closed by its specials, all of them laid end to end, the stream cut into rows of
// exactly row_len cells ("concatenate and chunk", the input of causal-LM pretraining), with next-token labels, a segment and a position plane.
//
// Additive (the reference has no counterpart; include/blingfiretokdll_amd.h IdsToStreamRowsBatchDevice is the specification).  Sequence q becomes
// the unit [bos] ids[0 .. n_q) [eos] of width w_q, every id and none dropped; W = the exclusive scan of the widths, T = W[nseq] the length of the
// stream S.  Row r is S[r * L .. (r + 1) * L): a unit runs over a row's edge into the next row.  The output IS the stream, so the fill works on
// the flat cell space in tiles of consecutive cells: a tile's first and last unit are found once per tile by a search of the whole W that a wave
// makes together (stream_probe / stream_narrow: 64 probes a round), the tile's slice of W is staged relative to the tile (StreamStaged), and a
// lane finds its unit there.  A slice longer than STREAM_STAGE_UNITS (runs of units of width 0 are unbounded) is searched in global memory between
// the tile's two bounds instead (StreamGlobal); both answer through the same calls, and the cell code is written once over either.
//
// Everything a lane decides is written once here as BF_HD code: bf_kernels_stream.hip runs it per lane, tests/hosttest compiles the same header
// for the host (test-only: the product library never cuts a stream on the CPU).  Plain C++, no HIP types.
#pragma once
#include <stdint.h>
#include "bf_rows.h"

// (a loop over a lane's cells is unrolled in the kernel, so that the cells stay in registers; the host build has no such pragma)
#if defined(__HIPCC__)
#define BF_STREAM_UNROLL _Pragma("unroll")
#else
#define BF_STREAM_UNROLL
#endif

namespace bfa {

constexpr int STREAM_DROP_LAST = 1;          // flags bit 0: the last incomplete row is dropped
constexpr int STREAM_POS_FROM_ROW = 2;       // flags bit 1: a unit that continues from the row before counts its positions from the row's edge
constexpr int STREAM_LABELS_WITHIN = 4;      // flags bit 2: a label that lies in another unit than its cell is ignore_label
constexpr int STREAM_FLAGS = 7;

// the tile geometry: a workgroup of STREAM_TILE_LANES lanes takes tiles of STREAM_TILE_LANES * C consecutive cells (C = 4 or 1 cells per lane)
constexpr int STREAM_TILE_LANES = 256;
constexpr int STREAM_WIDE_CELLS = 4;
constexpr int STREAM_STAGE_UNITS = 768;      // the most units a tile's staged slice may hold (9 KiB of LDS); a longer slice takes the global search
constexpr int STREAM_PROBES = 64;            // pieces a round of the wave's search cuts its range into: a probe per lane (stream_step shifts by its log2)
constexpr int64_t STREAM_MAX_IDS = 0x7fffffff - 2;       // a sequence of more ids is read as empty: the widths are int32

struct StreamSpec {
    int row_len, bos_id, eos_id, pad_id, ignore_label, flags;
    int lead, trail;                      // 1 when bos_id / eos_id are written
};

// fills `s`; false = the parameters are refused (BF_E_ARG)
BF_HD bool stream_spec(int row_len, int bos_id, int eos_id, int pad_id, int ignore_label, int flags, StreamSpec *s)
{
    if (row_len < 1 || row_len > ROWS_MAX_LEN || (flags & ~STREAM_FLAGS) != 0) return false;
    s->row_len = row_len; s->bos_id = bos_id; s->eos_id = eos_id; s->pad_id = pad_id; s->ignore_label = ignore_label; s->flags = flags;
    s->lead = bos_id >= 0 ? 1 : 0; s->trail = eos_id >= 0 ? 1 : 0;
    return true;
}

// the host-known bound of the row count, ceil((ids_len + (lead + trail) * nseq) / row_len): every id and every special in a cell of its own
BF_HD int64_t stream_rows_bound(const StreamSpec &s, int64_t ids_len, int64_t nseq)
{
    return (ids_len + (int64_t)(s.lead + s.trail) * nseq + s.row_len - 1) / s.row_len;
}

// the width of the unit of sequence [b, e) of the ids: a bad range (rows_seq_len) and a sequence of more than STREAM_MAX_IDS ids are read as empty
BF_HD int32_t stream_width(const StreamSpec &s, int64_t b, int64_t e, int64_t ids_len, bool *bad)
{
    int64_t n = rows_seq_len(b, e, ids_len, bad);
    if (n > STREAM_MAX_IDS) { n = 0; *bad = true; }
    return (int32_t)(s.lead + n + s.trail);
}

// the row count: ceil(T / L), with STREAM_DROP_LAST floor(T / L)
BF_HD int64_t stream_nrows(const StreamSpec &s, int64_t T) { return (s.flags & STREAM_DROP_LAST) ? T / s.row_len : (T + s.row_len - 1) / s.row_len; }

// the per-sequence pair: the cell where unit q begins
BF_HD void stream_seq_cell(const StreamSpec &s, int64_t Wq, int32_t *row, int32_t *col) { *row = (int32_t)(Wq / s.row_len); *col = (int32_t)(Wq % s.row_len); }

// ---- the unit search over the whole W, made by the 64 lanes of a wave together.  Wanted: the last q in [lo, hi) with W[q] <= t, where W[lo] <= t
// holds and hi is the end of the array or has W[hi] > t.  A round cuts the range into 64 pieces of `step` units: lane k probes
// stream_probe(lo, hi, k), the first unit of piece k + 1 (-1 = there is no such piece: it answers "no"), the ballot of "W[probe] <= t" goes to
// stream_narrow.  W is sorted, so the lanes that answer yes are the low ones and their count is the piece the answer lies in; the range shrinks
// 64-fold a round (2^31 units: six rounds, with shifts alone), and hi - lo == 1 ends the search with the answer lo.
BF_HD int64_t stream_step(int64_t lo, int64_t hi) { return (hi - lo + STREAM_PROBES - 1) >> 6; }
BF_HD int64_t stream_probe(int64_t lo, int64_t hi, int lane)
{
    const int64_t at = lo + (lane + 1) * stream_step(lo, hi);
    return at < hi ? at : -1;
}
BF_HD void stream_narrow(int64_t *lo, int64_t *hi, unsigned long long yes)
{
    const int64_t step = stream_step(*lo, *hi);
    int c = 0;
    for (unsigned long long m = yes; m; m &= m - 1) ++c;
    const int64_t nlo = *lo + c * step, nhi = nlo + step;
    *lo = nlo;
    if (nhi < *hi) *hi = nhi;
}

// the last q in [lo, hi) with W[q] <= t (W[lo] <= t holds): one lane's binary search, for a range a tile has bounded
BF_HD int64_t stream_find_unit(const int64_t *W, int64_t lo, int64_t hi, int64_t t)
{
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (W[mid] <= t) lo = mid; else hi = mid;
    }
    return lo;
}

// a unit as a cell sees it: its number, where it begins and ends in the stream, and delta = off[q] - W[q] - lead, which turns a stream position
// t that holds an id into the element ids[t + delta].  (delta is computed in unsigned arithmetic: the offsets of a bad range are anything.)
struct StreamUnit { int64_t q, w0, w1, delta; };
BF_HD int64_t stream_delta(int64_t off_q, int64_t Wq, int lead) { return (int64_t)((uint64_t)off_q - (uint64_t)Wq - (uint64_t)lead); }

// A tile's slice of W as the lanes read it.  Both sources answer at(t, u): the unit of stream position t, where u is a unit at or in front
// of it (a lane carries its unit from left to right and searches only where a cell left the unit of the cell before).
//
// StreamGlobal: the units [qa, qe] in global memory
struct StreamGlobal {
    const int64_t *W, *off; int64_t qa, qe; int lead;
    BF_HD StreamUnit load(int64_t q) const { return StreamUnit{q, W[q], W[q + 1], stream_delta(off[q], W[q], lead)}; }
    BF_HD StreamUnit first() const { return load(qa); }
    BF_HD StreamUnit at(int64_t t, const StreamUnit &u) const { return u.w1 > t ? u : load(stream_find_unit(W, u.q + 1, qe + 1, t)); }
};
// StreamStaged: the same units staged: wrel[i] = W[qa + i] - t0 for i = 0 .. n (n = qe - qa + 1 units, and the end of the last one), clamped
// from above (stream_wrel: a value behind the tile and the cell after it only has to stay there), delta[i] for i < n
BF_HD int32_t stream_wrel(int64_t Wq, int64_t t0) { const int64_t d = Wq - t0; return d > 0x7fffffff ? 0x7fffffff : (int32_t)d; }
struct StreamStaged {
    const int32_t *wrel; const int64_t *delta; int64_t t0, qa; int n;
    BF_HD StreamUnit load(int i) const { return StreamUnit{qa + i, t0 + wrel[i], t0 + wrel[i + 1], delta[i]}; }
    BF_HD StreamUnit first() const { return load(0); }
    BF_HD StreamUnit at(int64_t t, const StreamUnit &u) const
    {
        if (u.w1 > t) return u;
        const int32_t trel = (int32_t)(t - t0);
        int lo = (int)(u.q - qa) + 1, hi = n;
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (wrel[mid] <= trel) lo = mid; else hi = mid;
        }
        return load(lo);
    }
};

// the element of the stream at position t, which lies in unit u
BF_HD int32_t stream_elem(const StreamSpec &sp, int64_t t, const StreamUnit &u, const int32_t *ids)
{
    const int32_t bos = sp.bos_id, eos = sp.eos_id;            // (by value: a choice between the two fields' addresses would put the spec into scratch)
    const bool is_bos = sp.lead && t == u.w0, is_eos = sp.trail && t + 1 == u.w1;
    if (is_bos || is_eos) return is_bos ? bos : eos;
    return ids[t + u.delta];
}

struct StreamCell { int32_t id, seg, pos, label; };

// The C cells [t, t + C) of one lane, all in row r = t / L at places j .. j + C - 1, from a tile's source.  T = the length of the stream; f_hint =
// the unit of the first cell of the row when the row begins in front of the tile (t0_row < tile start), else ignored: a row that begins inside
// the tile finds it in the source.  want_label: labels are taken (the element one past the lane's cells is fetched only then).
// *first_seq / *first_pos: the row-first pair, valid when j == 0.  `tile0` = the first stream position the source covers.
template <int C, class Src>
BF_HD void stream_cells(const StreamSpec &sp, const Src &src, const int32_t *ids, int64_t T, int64_t tile0, int64_t f_hint, int64_t t, int j, bool want_label,
                        StreamCell *c, int32_t *first_seq, int32_t *first_pos)
{
    *first_seq = 0; *first_pos = 0;
    BF_STREAM_UNROLL
    for (int k = 0; k < C; ++k) c[k] = StreamCell{sp.pad_id, 0, 0, sp.ignore_label};
    if (t >= T) return;                                       // padding, and everything behind it in the lane
    const StreamUnit u0 = src.first();
    StreamUnit u = src.at(t, u0);
    const int64_t row0 = t - j;
    const int64_t f = j == 0 ? u.q : row0 < tile0 ? f_hint : src.at(row0, u0).q;
    if (j == 0) { *first_seq = (int32_t)u.q; *first_pos = (int32_t)(t - u.w0); }
    int32_t e = stream_elem(sp, t, u, ids);
    BF_STREAM_UNROLL
    for (int k = 0; k < C; ++k) {
        const int64_t tk = t + k;
        if (tk < T) {
            const int64_t x = tk - u.w0;
            c[k].id = e;
            c[k].seg = (int32_t)(u.q - f + 1);
            c[k].pos = (int32_t)(((sp.flags & STREAM_POS_FROM_ROW) && x > j + k) ? j + k : x);
            if (tk + 1 < T && (k < C - 1 || want_label)) {
                const int64_t q = u.q;
                u = src.at(tk + 1, u);
                e = stream_elem(sp, tk + 1, u, ids);
                if (!((sp.flags & STREAM_LABELS_WITHIN) && u.q != q)) c[k].label = e;
            }
        }
    }
}

} // namespace bfa
