// bf_mlmcaptest.cpp -- TEST-ONLY: the lane code of the capped MLM call (blingfire_amd/csrc/bf_mlm.h: the key, the compare, the threshold search, the
// "kept" predicate, the gather slot with its chunk carry) compiled for the host and driven in the lane partition of k_rows_mlm_cap: G lanes per
// row, three walks over the row's chunks (A: the word of every cell and the count; B: the search, one count over all chunks per round, only where
// the row does not fit; C: kept flags as a ballot of the group, slots by popcount + carry, the cells, the tail, the count).  A ballot is a loop over
// the group's lanes here.  With BF_MLMCAPTEST_MAIN the file is a program of its own over exactly sized heap arrays (tests build it with
// -fsanitize=address,undefined).
#include <stdint.h>
#include <stddef.h>
#include <vector>
#include "../../blingfire_amd/csrc/bf_rows.h"
#include "../../blingfire_amd/csrc/bf_mlm.h"
#include "rowwalk_emu.h"

using namespace bfa;

namespace {

// phases B and C over the words of one row: kept[j], slot[j] (of kept cells) -> the number of kept cells
int cap_row(const uint64_t *words, int row_len, int G, int P, uint8_t *kept, int32_t *slot)
{
    const int nchunks = (row_len + G - 1) / G, head_bits = mlm_cap_head_bits(row_len);
    auto word = [&](int c, int l) { return c * G + l < row_len ? words[c * G + l] : MLM_CAP_NONE; };
    int selected = 0;
    for (int c = 0; c < nchunks; ++c) for (int l = 0; l < G; ++l) selected += word(c, l) != MLM_CAP_NONE;
    uint64_t T = 0;
    if (selected > P) {
        for (int i = mlm_cap_rounds(head_bits) - 1; i >= 0; --i) {
            const uint64_t probe = mlm_cap_probe(T, i, head_bits);
            int n = 0;
            for (int c = 0; c < nchunks; ++c) for (int l = 0; l < G; ++l) n += mlm_cap_below(word(c, l), probe) ? 1 : 0;
            T = mlm_cap_take(T, probe, n, P);
            if (n == P) break;                                // the kernel's early end
        }
    }
    MlmCapCarry slots = mlm_cap_carry_none();
    for (int c = 0; c < nchunks; ++c) {
        uint64_t kept_lanes = 0;
        for (int l = 0; l < G; ++l) if (c * G + l < row_len && mlm_cap_kept(word(c, l), selected, P, T)) kept_lanes |= (uint64_t)1 << l;
        for (int l = 0; l < G && c * G + l < row_len; ++l) {
            const bool k = ((kept_lanes >> l) & 1) != 0;
            kept[c * G + l] = k ? 1 : 0;
            slot[c * G + l] = k ? mlm_cap_slot(slots, kept_lanes, l) : -1;
        }
        slots = mlm_cap_carry_next(slots, kept_lanes);
    }
    return slots.kept;
}

} // namespace

extern "C" {

// the search alone over words chosen by hand (one row): kept_out[j] 0 / 1, slot_out[j] the gather slot or -1; returns the kept cells, -1 = refused
int bft_mlmcap_search(const uint64_t *words, int row_len, int group, int P, uint8_t *kept_out, int32_t *slot_out)
{
    if (row_len < 1 || row_len > MLM_CAP_MAX_LEN || P < 1 || group < 1 || group > 64 || (group & (group - 1))) return -1;
    return cap_row(words, row_len, group, P, kept_out, slot_out);
}

uint64_t bft_mlmcap_key(uint32_t w3, int h) { return mlm_cap_key(w3, h); }

// k_rows_mlm_cap over nrows rows with `group` lanes per row (0 = span_group(row_len)).  The arguments of bft_mlm_rows, then max_pred > 0 and the
// three gathered outputs; any output may be NULL; ids_out may be `rows`.  Returns 0, or -1 = refused.
int bft_mlmcap_rows(const int32_t *rows, int row_len, int64_t nrows, int64_t row_base, const uint8_t *mask, const int32_t *seg, const int32_t *S, const int32_t *E,
                    int nspecial, const int32_t *special_ids, double select_prob, double mask_prob, double random_prob, int mask_id, int rand_lo, int rand_hi,
                    int ignore_label, uint64_t seed, uint32_t epoch, int32_t *ids_out, int32_t *labels_out, int max_pred, int32_t *pred_cell, int32_t *pred_label,
                    int32_t *pred_count, int group)
{
    MlmSpec sp;
    if (row_len < 1 || row_len > MLM_CAP_MAX_LEN || nrows < 0 || (S != nullptr) != (E != nullptr) || max_pred < 1 || max_pred > MLM_CAP_MAX_PRED) return -1;
    if (!ids_out && !labels_out && !pred_cell && !pred_label && !pred_count) return -1;
    if (!mlm_spec(nspecial, special_ids, select_prob, mask_prob, random_prob, mask_id, rand_lo, rand_hi, ignore_label, seed, epoch, &sp)) return -1;
    const int G = group > 0 ? group : span_group(row_len), P = max_pred;
    const bool ww = S != nullptr;
    std::vector<uint64_t> words((size_t)row_len);
    std::vector<uint8_t> kept((size_t)row_len);
    std::vector<int32_t> slot((size_t)row_len);
    std::vector<EmuHeadCell> cell((size_t)G);
    std::vector<int> hd((size_t)G);
    for (int64_t r = 0; r < nrows; ++r) {
        const int64_t base = r * row_len;
        MlmCarry carry = mlm_carry_none();
        for (int j0 = 0; j0 < row_len; j0 += G) {             // A
            for (int l = 0; l < G; ++l) {
                const int j = j0 + l;
                const bool in = j < row_len;
                cell[(size_t)l] = EmuHeadCell{in && ww ? S[base + j] : -1, in && ww ? E[base + j] : 0,
                                              in && mlm_eligible(sp, rows[base + j], mask ? mask[base + j] : (uint8_t)1, seg ? seg[base + j] : 1)};
                hd[(size_t)l] = j;
            }
            if (ww) emu_chunk_head(cell.data(), G, j0, carry, hd.data());
            for (int l = 0; l < G && j0 + l < row_len; ++l)
                words[(size_t)(j0 + l)] = cell[(size_t)l].eligible ? mlm_cap_word(sp, true, mlm_draw(sp, r + row_base, hd[(size_t)l]), hd[(size_t)l]) : MLM_CAP_NONE;
        }
        const int n = cap_row(words.data(), row_len, G, P, kept.data(), slot.data());          // B, C
        for (int j = 0; j < row_len; ++j) {
            const int32_t id = rows[base + j];                // (read before the cell is written: in place)
            if (ids_out) ids_out[base + j] = kept[(size_t)j] ? mlm_kept_id(sp, r + row_base, j, id) : id;
            if (labels_out) labels_out[base + j] = kept[(size_t)j] ? id : sp.ignore_label;
            if (kept[(size_t)j]) {
                if (pred_cell) pred_cell[r * P + slot[(size_t)j]] = j;
                if (pred_label) pred_label[r * P + slot[(size_t)j]] = id;
            }
        }
        for (int k = n; k < P; ++k) {
            if (pred_cell) pred_cell[r * P + k] = 0;
            if (pred_label) pred_label[r * P + k] = sp.ignore_label;
        }
        if (pred_count) pred_count[r] = n;
    }
    return 0;
}

} // extern "C"

#ifdef BF_MLMCAPTEST_MAIN
#include <cstdio>

// Exactly sized heap arrays (a read or a write past them is the sanitizer's to find), every group size, both forms, in place.  Checked here: only
// what needs no second implementation -- every group size gives what one lane per row gives; the count is at most P and is the number of labels; the
// gathered cells rise, are labelled cells, and carry the original id; the tail holds 0 and the ignore label; with P >= row_len nothing is dropped
// (labels equal a second run at a larger P); a hand-made row of the search.
static int run_case(int L, int64_t R, bool ww, int P)
{
    const size_t n = (size_t)(R * L), np = (size_t)(R * P);
    std::vector<int32_t> rows(n), seg(n), S(n), E(n);
    std::vector<uint8_t> mask(n);
    const int32_t specials[3] = {101, 102, 0};
    uint32_t x = 4321u + (uint32_t)L * 7919u + (uint32_t)P;
    auto rnd = [&x]() { x = x * 1664525u + 1013904223u; return x >> 8; };
    for (int64_t r = 0; r < R; ++r) {
        int32_t at = 0;
        for (int j = 0; j < L; ++j) {
            const size_t c = (size_t)(r * L + j);
            rows[c] = rnd() % 20 == 0 ? specials[rnd() % 3] : 1000 + (int32_t)(rnd() % 29000);
            mask[c] = rnd() % 10 != 0; seg[c] = (int32_t)(rnd() % 4);
            if (r > 0 && rnd() % 3 == 0) at += 2;
            const int32_t len = 1 + (int32_t)(rnd() % 3);
            S[c] = at; E[c] = at + len - 1; at += len;
            if (r > 0 && rnd() % 12 == 0) { S[c] = -1; E[c] = -1; }
        }
    }
    std::vector<int32_t> ids1(n), lab1(n), cell1(np), pl1(np), cnt1((size_t)R), ids(n), lab(n), cell(np), pl(np), cnt((size_t)R);
    auto call = [&](const int32_t *src, int32_t *io, int32_t *lo, int32_t *co, int32_t *po, int32_t *no, int p, int g) {
        return bft_mlmcap_rows(src, L, R, ((int64_t)1 << 33) + 5, mask.data(), seg.data(), ww ? S.data() : nullptr, ww ? E.data() : nullptr, 3, specials, 0.4, 0.8, 0.1, 103,
                               1000, 30522, -100, 0x123456789abcdefull, 3, io, lo, p, co, po, no, g);
    };
    if (call(rows.data(), ids1.data(), lab1.data(), cell1.data(), pl1.data(), cnt1.data(), P, 1) != 0) return 1;
    for (int g = 0; g <= 64; g = g ? g * 2 : 1) {
        if (call(rows.data(), ids.data(), lab.data(), cell.data(), pl.data(), cnt.data(), P, g) != 0) return 1;
        if (ids != ids1 || lab != lab1 || cell != cell1 || pl != pl1 || cnt != cnt1) return 1;
        std::vector<int32_t> inplace(rows), pl2(np);
        if (call(inplace.data(), inplace.data(), nullptr, nullptr, pl2.data(), nullptr, P, g) != 0 || inplace != ids1 || pl2 != pl1) return 1;      // in place
        std::vector<int32_t> only((size_t)R);
        if (call(rows.data(), nullptr, nullptr, nullptr, nullptr, only.data(), P, g) != 0 || only != cnt1) return 1;                             // the count alone
    }
    for (int64_t r = 0; r < R; ++r) {
        int labelled = 0;
        for (int j = 0; j < L; ++j) labelled += lab1[(size_t)(r * L + j)] != -100;
        if (cnt1[(size_t)r] != labelled || labelled > P) return 1;
        for (int k = 0; k < P; ++k) {
            const size_t s = (size_t)(r * P + k);
            if (k >= labelled) { if (cell1[s] != 0 || pl1[s] != -100) return 1; continue; }
            if (cell1[s] < 0 || cell1[s] >= L || (k > 0 && cell1[s] <= cell1[s - 1])) return 1;
            const size_t c = (size_t)(r * L + cell1[s]);
            if (lab1[c] != rows[c] || pl1[s] != rows[c]) return 1;
        }
    }
    if (P >= L) {                                             // nothing to drop: a larger cap changes nothing in ids and labels
        std::vector<int32_t> ids2(n), lab2(n);
        if (bft_mlmcap_rows(rows.data(), L, R, ((int64_t)1 << 33) + 5, mask.data(), seg.data(), ww ? S.data() : nullptr, ww ? E.data() : nullptr, 3, specials, 0.4, 0.8, 0.1, 103,
                            1000, 30522, -100, 0x123456789abcdefull, 3, ids2.data(), lab2.data(), P + 7, nullptr, nullptr, nullptr, 0) != 0 || ids2 != ids1 || lab2 != lab1) return 1;
    }
    return 0;
}

static int check_search()
{
    // units (cells: key) 0-1: (5, 0)   2: (5, 2)   3-5: (1, 3)   6: none   7: (9, 7): in key order 3-5, 0-1, 2, 7 with prefix sums 3, 5, 6, 7
    const uint64_t N = MLM_CAP_NONE;
    const uint64_t w[8] = {mlm_cap_key(5, 0), mlm_cap_key(5, 0), mlm_cap_key(5, 2), mlm_cap_key(1, 3), mlm_cap_key(1, 3), mlm_cap_key(1, 3), N, mlm_cap_key(9, 7)};
    const int want[8] = {0, 0, 3, 3, 5, 6, 7, 7};             // kept cells at P = 1 .. 8 (P = 4: the unit 0-1 does not fit, and cell 2 behind it is not taken)
    for (int g = 1; g <= 64; g *= 2)
        for (int P = 1; P <= 8; ++P) {
            std::vector<uint8_t> kept(8);
            std::vector<int32_t> slot(8);
            if (bft_mlmcap_search(w, 8, g, P, kept.data(), slot.data()) != want[P - 1]) return 1;
        }
    return 0;
}

int main()
{
    if (check_search()) { fprintf(stderr, "FAILED: the search\n"); return 1; }
    const int Ls[10] = {1, 3, 4, 31, 32, 33, 64, 65, 130, 200};
    int64_t cases = 0;
    for (int L : Ls) for (int ww = 0; ww <= 1; ++ww) {
        const int Ps[5] = {1, 2, L / 8 > 1 ? L / 8 : 1, L, L + 5};
        for (int P : Ps) {
            if (run_case(L, 9, ww != 0, P)) { fprintf(stderr, "FAILED: L %d whole-word %d P %d\n", L, ww, P); return 1; }
            ++cases;
        }
    }
    printf("mlmcap ok: %lld cases\n", (long long)cases);
    return 0;
}
#endif
