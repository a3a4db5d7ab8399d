// bf_charpostest.cpp -- TEST-ONLY: the lane code of the offset conversions (blingfire_amd/csrc/bf_charpos.h: the pieces of the two masks, the
// chunk weights, G, the document search, the chunk search and the bisection inside a chunk) compiled for the host and driven in the kernels' own
// partition: a wave of 64 lanes takes 1024 bytes, a lane 16, four lanes' pieces make a chunk's masks; P is the exclusive scan of the weights; a
// lane per document; a lane per item, the documents of a wave's first and last item found by the wave's 64 probes a round.  A shuffle is an index
// into the wave's arrays here, a ballot a loop over its lanes.  With BF_CHARPOSTEST_MAIN the file is a program of its own over exactly sized heap
// arrays (tests build it with -fsanitize=address,undefined).
#include <stdint.h>
#include <stddef.h>
#include <string.h>
#include <vector>
#include "../../blingfire_amd/csrc/bf_batch.h"
#include "../../blingfire_amd/csrc/bf_stream.h"
#include "../../blingfire_amd/csrc/bf_charpos.h"

using namespace bfa;

namespace {

// the wave's search of bf_kernels_charpos.hip (wave_find_doc)
int64_t wave_find_doc(const int64_t *off, int64_t n, int64_t t)
{
    int64_t lo = 0, hi = n;
    while (hi - lo > 1) {
        unsigned long long yes = 0;
        for (int lane = 0; lane < 64; ++lane) {
            const int64_t at = stream_probe(lo, hi, lane);
            if (at >= 0 && off[at] <= t) yes |= 1ull << lane;
        }
        stream_narrow(&lo, &hi, yes);
    }
    return lo;
}

} // namespace

extern "C" {

// the two masks and the weights of a text, as k_char_index leaves them: lead / four / counts have charpos_nchunks(total) entries (four may be NULL)
void bft_charpos_index(const uint8_t *text, int64_t total, uint64_t *lead, uint64_t *four, int32_t *counts)
{
    const int64_t nchunks = charpos_nchunks(total), tiles = (total + CHARPOS_WAVE_BYTES - 1) / CHARPOS_WAVE_BYTES;
    for (int64_t tile = 0; tile < tiles; ++tile) {
        uint64_t pl[64], pf[64];
        for (int lane = 0; lane < 64; ++lane) {
            const int64_t at = tile * CHARPOS_WAVE_BYTES + lane * CHARPOS_LANE_BYTES;
            uint32_t w[4] = {0x80808080u, 0x80808080u, 0x80808080u, 0x80808080u};
            if (at + CHARPOS_LANE_BYTES <= total) memcpy(w, text + at, CHARPOS_LANE_BYTES);
            else if (at < total) charpos_tail_words(text, at, total, w);
            uint32_t l16, f16;
            charpos_piece(w, &l16, &f16);
            pl[lane] = charpos_place(l16, lane); pf[lane] = four ? charpos_place(f16, lane) : 0;
        }
        for (int step = 1; step <= 2; step <<= 1) {           // the two exchanges
            uint64_t nl[64], nf[64];
            for (int lane = 0; lane < 64; ++lane) { nl[lane] = pl[lane] | pl[lane ^ step]; nf[lane] = pf[lane] | pf[lane ^ step]; }
            memcpy(pl, nl, sizeof pl); memcpy(pf, nf, sizeof pf);
        }
        for (int lane = 0; lane < 64; lane += 4) {
            const int64_t c = tile * (CHARPOS_WAVE_BYTES / CHARPOS_CHUNK) + (lane >> 2);
            if (c >= nchunks) continue;
            lead[c] = pl[lane];
            if (four) four[c] = pf[lane];
            counts[c] = charpos_chunk_count(pl[lane], pf[lane]);
        }
    }
}

// ByteToCharOffsetsBatchDevice (dir 0) / CharToByteOffsetsBatchDevice (dir 1) without a handle: the arguments, the refusals (-1) and the outputs.
// *status_out (may be NULL) gets the status word.
int bft_charpos(int dir, const uint8_t *text, const int64_t *doc_off, int64_t ndocs, int64_t total, const int64_t *item_off, int64_t items_cap, const int32_t *starts,
                const int32_t *ends, int unit, int flags, int32_t *starts_out, int32_t *ends_out, int32_t *doc_units, int *status_out)
{
    if ((unit != CHARPOS_UNIT_CHAR && unit != CHARPOS_UNIT_UTF16) || (flags & ~CHARPOS_FLAGS) != 0 || ndocs < 0 || total < 0 || items_cap < 0) return -1;
    if ((starts != nullptr) != (starts_out != nullptr) || (ends != nullptr) != (ends_out != nullptr)) return -1;
    if (!doc_off || (total > 0 && !text)) return -1;
    const int64_t items_bound = ndocs == 0 ? 0 : item_off ? items_cap : (items_cap < ndocs ? items_cap : ndocs);
    const bool want_items = starts_out || ends_out;
    if (items_bound > 0 && !want_items && !doc_units) return -1;
    int status = 0;
    const int64_t nchunks = charpos_nchunks(total);
    std::vector<uint64_t> lead((size_t)nchunks), four(unit == CHARPOS_UNIT_UTF16 ? (size_t)nchunks : 0);
    std::vector<int32_t> counts((size_t)nchunks);
    std::vector<int64_t> P((size_t)nchunks + 1);
    bft_charpos_index(text, total, lead.data(), unit == CHARPOS_UNIT_UTF16 ? four.data() : nullptr, counts.data());
    P[0] = 0;
    for (int64_t c = 0; c < nchunks; ++c) P[(size_t)c + 1] = P[(size_t)c] + counts[(size_t)c];
    const CharIndex ix{lead.data(), unit == CHARPOS_UNIT_UTF16 ? four.data() : nullptr, P.data()};
    for (int64_t d = 0; d < ndocs; ++d) {                     // k_char_docs
        const CharDoc doc = charpos_doc(doc_off[d], doc_off[d + 1], total);
        if (doc.bad) status |= BF_STATUS_BAD_OFFSETS;
        if (doc_units) doc_units[d] = charpos_units32(charpos_units(ix, doc));
    }
    if (want_items && items_bound > 0) {                       // k_char_fwd / k_char_inv
        const int64_t all = item_off ? item_off[ndocs] : ndocs;
        const int64_t n = all < items_cap ? all : items_cap;
        for (int64_t i0 = 0; i0 < n; i0 += 64) {
            const int64_t last = i0 + 63 < n ? i0 + 63 : n - 1;
            int64_t dlo = 0, dhi = 0;
            if (item_off) { dlo = wave_find_doc(item_off, ndocs, i0); dhi = wave_find_doc(item_off, ndocs, last); }
            for (int lane = 0; lane < 64; ++lane) {
                const int64_t i = i0 + lane;
                if (i >= n) continue;
                int64_t d = i;
                bool held = true;
                if (item_off) {
                    d = charpos_item_doc(item_off, dlo, dhi, i);
                    held = item_off[d] <= i && i < item_off[d + 1];
                }
                bool bad = !held;
                int32_t s = -1, e = -1;
                if (held) {
                    const CharDoc doc = charpos_doc(doc_off[d], doc_off[d + 1], total);
                    const int64_t Gb = doc.n > 0 ? charpos_G(ix, doc.b) : 0;
                    const int64_t U = dir == CHARPOS_INV ? charpos_units(ix, doc) : 0;
                    if (starts) s = charpos_convert(ix, doc, Gb, U, dir, flags, false, starts[i], &bad);
                    if (ends) e = charpos_convert(ix, doc, Gb, U, dir, flags, true, ends[i], &bad);
                }
                if (starts_out) starts_out[i] = s;
                if (ends_out) ends_out[i] = e;
                if (bad) status |= BF_STATUS_BAD_OFFSETS;
            }
        }
    }
    if (status_out) *status_out = status;
    return 0;
}

} // extern "C"

#ifdef BF_CHARPOSTEST_MAIN
#include <cstdio>

// Exactly sized heap arrays (a read or a write past them is the sanitizer's to find).  Checked here against the definition read byte by byte:
// C_d and B_d at every position of every document, both units, the four end conventions, in place and out of place, at totals around the
// chunk and the wave edges.
static int weight(uint8_t b, int unit) { return (b & 0xC0) == 0x80 ? 0 : (unit == 1 && b >= 0xF0) ? 2 : 1; }

static int run_case(int64_t total, int ndocs, uint32_t seed)
{
    uint32_t x = seed;
    auto rnd = [&x]() { x = x * 1664525u + 1013904223u; return x >> 8; };
    std::vector<uint8_t> text((size_t)total);
    static const uint8_t kinds[8] = {'a', 0xC3, 0xA9, 0xE2, 0x82, 0xF0, 0x9F, 0xFF};
    for (auto &b : text) b = kinds[rnd() % 8];
    std::vector<int64_t> off((size_t)ndocs + 1, 0);
    for (int d = 1; d < ndocs; ++d) off[(size_t)d] = total ? (int64_t)(rnd() % (uint32_t)(total + 1)) : 0;
    off[(size_t)ndocs] = total;
    for (int d = 1; d <= ndocs; ++d) if (off[(size_t)d] < off[(size_t)d - 1]) off[(size_t)d] = off[(size_t)d - 1];
    for (int unit = 0; unit <= 1; ++unit)
        for (int dir = 0; dir <= 1; ++dir)
            for (int flags = 0; flags <= 3; ++flags) {
                std::vector<int32_t> vals, want_s, want_e;
                std::vector<int64_t> ioff((size_t)ndocs + 1, 0);
                std::vector<int32_t> want_units((size_t)ndocs);
                int want_status = 0;
                for (int d = 0; d < ndocs; ++d) {
                    const int64_t b = off[(size_t)d], n = off[(size_t)d + 1] - b;
                    std::vector<int64_t> C((size_t)n + 1, 0), B;
                    for (int64_t i = 0; i < n; ++i) C[(size_t)i + 1] = C[(size_t)i] + weight(text[(size_t)(b + i)], unit);
                    const int64_t U = C[(size_t)n];
                    for (int64_t k = 0; k <= U; ++k) { int64_t i = 0; if (k == U) i = n; else while (!(C[(size_t)i + 1] > k)) ++i; B.push_back(i); }
                    const std::vector<int64_t> &F = dir == 0 ? C : B;
                    want_units[(size_t)d] = (int32_t)U;
                    for (int64_t v = -1; v <= (int64_t)F.size(); ++v) {
                        vals.push_back((int32_t)v);
                        const int64_t xe = v + ((flags & 1) ? 0 : 1);
                        if (v < 0) { want_s.push_back(-1); want_e.push_back(-1); continue; }
                        if (v >= (int64_t)F.size()) { want_s.push_back(-1); want_status = 8; } else want_s.push_back((int32_t)F[(size_t)v]);
                        if (xe >= (int64_t)F.size()) { want_e.push_back(-1); want_status = 8; } else want_e.push_back((int32_t)(F[(size_t)xe] - ((flags & 2) ? 0 : 1)));
                    }
                    ioff[(size_t)d + 1] = (int64_t)vals.size();
                }
                const int64_t n_items = (int64_t)vals.size();
                std::vector<int32_t> s_out((size_t)n_items), e_out((size_t)n_items), units((size_t)ndocs), in_s(vals), in_e(vals);
                int status = -1;
                if (bft_charpos(dir, text.data(), off.data(), ndocs, total, ioff.data(), n_items, vals.data(), vals.data(), unit, flags, s_out.data(), e_out.data(), units.data(),
                                &status) != 0) return 1;
                if (s_out != want_s || e_out != want_e || units != want_units || status != want_status) return 1;
                if (bft_charpos(dir, text.data(), off.data(), ndocs, total, ioff.data(), n_items, in_s.data(), in_e.data(), unit, flags, in_s.data(), in_e.data(), nullptr,
                                &status) != 0) return 1;
                if (in_s != want_s || in_e != want_e) return 1;             // in place
            }
    return 0;
}

int main()
{
    const int64_t totals[] = {0, 1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 1039, 1040, 2047, 2049, 5000};
    int64_t cases = 0;
    for (int64_t total : totals)
        for (int ndocs : {0, 1, 2, 7, 40}) {
            if (run_case(total, ndocs, (uint32_t)(total * 131 + ndocs))) { fprintf(stderr, "FAILED: total %lld ndocs %d\n", (long long)total, ndocs); return 1; }
            ++cases;
        }
    printf("charpos ok: %lld cases\n", (long long)cases);
    return 0;
}
#endif
