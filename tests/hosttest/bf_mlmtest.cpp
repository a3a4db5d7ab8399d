// bf_mlmtest.cpp -- TEST-ONLY: the lane code of the MLM masking call (blingfire_amd/csrc/bf_mlm.h: Philox, thresholds, eligibility, the continuation
// predicate, the head scan with its carry, the decision) compiled for the host and driven in the lane partition of k_rows_mlm: G lanes per row, a
// row walked in chunks of G cells, the whole-word head of a chunk from rowwalk_emu.h.  With BF_MLMTEST_MAIN the file is a program of its own over exactly sized heap arrays
// (tests build it with -fsanitize=address,undefined).
#include <stdint.h>
#include <stddef.h>
#include <vector>
#include "../../blingfire_amd/csrc/bf_rows.h"
#include "../../blingfire_amd/csrc/bf_mlm.h"
#include "rowwalk_emu.h"

using namespace bfa;

extern "C" {

void bft_philox(const uint32_t *c, const uint32_t *k, uint32_t *out)
{
    const Philox4 w = philox4x32_10(c[0], c[1], c[2], c[3], k[0], k[1]);
    for (int i = 0; i < 4; ++i) out[i] = w.v[i];
}

// the three thresholds (Ts, Tm, Tm + Tr) as the call computes them; -1 = the parameters are refused
int bft_mlm_thresholds(double select_prob, double mask_prob, double random_prob, int rand_lo, int rand_hi, uint64_t *out)
{
    MlmSpec s;
    if (!mlm_spec(0, nullptr, select_prob, mask_prob, random_prob, 0, rand_lo, rand_hi, 0, 0, 0, &s)) return -1;
    out[0] = s.t_select; out[1] = s.t_mask; out[2] = s.t_mask_random;
    return 0;
}

// k_rows_mlm over nrows rows with `group` lanes per row (0 = span_group(row_len), the kernel's choice; any power of two up to 64 otherwise).
// row_base is added to the row index the generator sees.  S / E both NULL: token masking.  ids_out may be `rows`.  Returns 0, or -1 = refused.
int bft_mlm_rows(const int32_t *rows, int row_len, int64_t nrows, int64_t row_base, const uint8_t *mask, const int32_t *seg, const int32_t *S, const int32_t *E,
                 int nspecial, const int32_t *special_ids, double select_prob, double mask_prob, double random_prob, int mask_id, int rand_lo, int rand_hi,
                 int ignore_label, uint64_t seed, uint32_t epoch, int32_t *ids_out, int32_t *labels_out, int group)
{
    MlmSpec sp;
    if (row_len < 1 || row_len > MLM_MAX_LEN || nrows < 0 || (S != nullptr) != (E != nullptr) || (!ids_out && !labels_out)) return -1;
    if (!mlm_spec(nspecial, special_ids, select_prob, mask_prob, random_prob, mask_id, rand_lo, rand_hi, ignore_label, seed, epoch, &sp)) return -1;
    const int G = group > 0 ? group : span_group(row_len);
    const bool ww = S != nullptr;
    std::vector<EmuHeadCell> cell((size_t)G);
    std::vector<int32_t> id((size_t)G);
    std::vector<int> h((size_t)G);
    for (int64_t r = 0; r < nrows; ++r) {
        const int64_t base = r * row_len;
        MlmCarry carry = mlm_carry_none();
        for (int j0 = 0; j0 < row_len; j0 += G) {
            for (int l = 0; l < G; ++l) {                 // every lane loads its own cell
                const int j = j0 + l;
                cell[(size_t)l] = EmuHeadCell{-1, 0, false};
                id[(size_t)l] = 0; h[(size_t)l] = j;
                if (j >= row_len) continue;
                id[(size_t)l] = rows[base + j];
                cell[(size_t)l].eligible = mlm_eligible(sp, id[(size_t)l], mask ? mask[base + j] : (uint8_t)1, seg ? seg[base + j] : 1);
                if (ww) { cell[(size_t)l].S = S[base + j]; cell[(size_t)l].E = E[base + j]; }
            }
            if (ww) emu_chunk_head(cell.data(), G, j0, carry, h.data());
            for (int l = 0; l < G && j0 + l < row_len; ++l) {
                int32_t id_out, label;
                mlm_decide(sp, r + row_base, j0 + l, h[(size_t)l], id[(size_t)l], cell[(size_t)l].eligible, &id_out, &label);
                if (ids_out) ids_out[base + j0 + l] = id_out;
                if (labels_out) labels_out[base + j0 + l] = label;
            }
        }
    }
    return 0;
}

} // extern "C"

#ifdef BF_MLMTEST_MAIN
#include <cstdio>

// Rows, masks and planes on exactly sized heap arrays (a read or a write past them is the sanitizer's to find), every group size, token and
// whole-word form, in place and out of place.  Checked here: only what needs no second implementation -- the three known answers of the
// generator; every group size gives what one lane per row gives; an unselected or ineligible cell keeps its id and gets the ignore label; a
// label is the id that was there; a masked id is the mask id, the old id or an id of the random range; with probability 1 / 0 every / no
// eligible cell is labelled; the cells of a unit are labelled together.
static int check_philox()
{
    const uint32_t c[3][4] = {{0, 0, 0, 0}, {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu}, {0x243f6a88u, 0x85a308d3u, 0x13198a2eu, 0x03707344u}};
    const uint32_t k[3][2] = {{0, 0}, {0xffffffffu, 0xffffffffu}, {0xa4093822u, 0x299f31d0u}};
    const uint32_t want[3][4] = {{0x6627e8d5u, 0xe169c58du, 0xbc57ac4cu, 0x9b00dbd8u}, {0x408f276du, 0x41c83b0eu, 0xa20bc7c6u, 0x6d5451fdu},
                                 {0xd16cfe09u, 0x94fdccebu, 0x5001e420u, 0x24126ea1u}};
    for (int i = 0; i < 3; ++i) {
        uint32_t out[4];
        bft_philox(c[i], k[i], out);
        for (int q = 0; q < 4; ++q) if (out[q] != want[i][q]) return 1;
    }
    return 0;
}

static int run_case(int L, int64_t R, bool ww, double ps, double pm, double pr, int nspecial)
{
    const size_t n = (size_t)(R * L);
    std::vector<int32_t> rows(n), seg(n), S(n), E(n);
    std::vector<uint8_t> mask(n);
    const int32_t specials[8] = {101, 102, 0, 5, 6, 7, 8, 9};
    uint32_t x = 12345u + (uint32_t)L * 7919u;
    auto rnd = [&x]() { x = x * 1664525u + 1013904223u; return x >> 8; };
    for (int64_t r = 0; r < R; ++r) {
        int32_t at = 0;
        for (int j = 0; j < L; ++j) {
            const size_t c = (size_t)(r * L + j);
            rows[c] = rnd() % 20 == 0 ? specials[rnd() % 8] : 1000 + (int32_t)(rnd() % 29000);
            mask[c] = rnd() % 10 != 0; seg[c] = (int32_t)(rnd() % 4);
            if (r > 0 && rnd() % 4 == 0) at += 2;        // row 0: byte-adjacent from end to end
            const int32_t len = 1 + (int32_t)(rnd() % 3);
            S[c] = at; E[c] = at + len - 1; at += len;
            if (r > 0 && rnd() % 12 == 0) { S[c] = -1; E[c] = -1; }
            if (r > 0 && rnd() % 40 == 0) { S[c] = 0; E[c] = 0x7fffffff; at = 0; }          // an end that must not wrap
        }
    }
    std::vector<int32_t> ids1(n), lab1(n), ids(n), lab(n);
    auto call = [&](const int32_t *src, int32_t *io, int32_t *lo, int g) {
        return bft_mlm_rows(src, L, R, ((int64_t)1 << 33) + 5, mask.data(), seg.data(), ww ? S.data() : nullptr, ww ? E.data() : nullptr, nspecial, specials, ps, pm, pr, 103,
                            1000, 30522, -100, 0x123456789abcdefull, 3, io, lo, g);
    };
    if (call(rows.data(), ids1.data(), lab1.data(), 1) != 0) return 1;
    for (int g = 0; g <= 64; g = g ? g * 2 : 1) {
        if (call(rows.data(), ids.data(), lab.data(), g) != 0 || ids != ids1 || lab != lab1) return 1;
        std::vector<int32_t> inplace(rows), only(n);
        if (call(inplace.data(), inplace.data(), nullptr, g) != 0 || inplace != ids1) return 1;          // in place, labels not taken
        if (call(rows.data(), nullptr, only.data(), g) != 0 || only != lab1) return 1;                   // ids not taken
    }
    for (int64_t r = 0; r < R; ++r)
        for (int j = 0; j < L; ++j) {
            const size_t c = (size_t)(r * L + j);
            bool special = false;
            for (int k = 0; k < nspecial; ++k) special = special || rows[c] == specials[k];
            const bool el = mask[c] != 0 && seg[c] != 0 && !special;
            const bool labelled = lab1[c] != -100;
            if (labelled && (!el || lab1[c] != rows[c])) return 1;
            if (!labelled && ids1[c] != rows[c]) return 1;
            if (labelled && ids1[c] != 103 && ids1[c] != rows[c] && (ids1[c] < 1000 || ids1[c] >= 30522)) return 1;
            if (el && ps == 1.0 && !labelled) return 1;
            if (ps == 0.0 && labelled) return 1;
            if (labelled && pm == 1.0 && ids1[c] != 103) return 1;
            if (ww && j > 0) {                           // cells of one unit: labelled together
                const size_t b = c - 1;
                bool sb = false;
                for (int k = 0; k < nspecial; ++k) sb = sb || rows[b] == specials[k];
                const bool elb = mask[b] != 0 && seg[b] != 0 && !sb;
                if (el && elb && S[b] >= 0 && S[c] >= 0 && (int64_t)S[c] - 1 == (int64_t)E[b] && labelled != (lab1[b] != -100)) return 1;
            }
        }
    return 0;
}

int main()
{
    if (check_philox()) { fprintf(stderr, "FAILED: philox known answers\n"); return 1; }
    uint64_t t[3];
    if (bft_mlm_thresholds(1.0, 0.5, 0.5, 0, 1, t) != 0 || t[0] != 4294967296ull || t[1] != 2147483648ull || t[2] != 4294967296ull) { fprintf(stderr, "FAILED: thresholds\n"); return 1; }
    if (bft_mlm_thresholds(0.5, 0.6, 0.5, 0, 1, t) != -1 || bft_mlm_thresholds(0.5, 0.5, 0.1, 5, 5, t) != -1 || bft_mlm_thresholds(__builtin_nan(""), 0.5, 0.1, 0, 1, t) != -1 ||
        bft_mlm_thresholds(0.5, 1.0, 0.0, 5, 5, t) != 0) { fprintf(stderr, "FAILED: refused parameters\n"); return 1; }
    const int Ls[10] = {1, 3, 4, 31, 32, 33, 64, 65, 130, 200};
    const double probs[4][3] = {{0.15, 0.8, 0.1}, {1.0, 1.0, 0.0}, {0.0, 0.8, 0.1}, {1.0, 0.0, 1.0}};
    int64_t cases = 0;
    for (int L : Ls) for (int ww = 0; ww <= 1; ++ww) for (int k = 0; k < 4; ++k) for (int nspecial = 0; nspecial <= 8; nspecial += 8) {
        if (run_case(L, 9, ww != 0, probs[k][0], probs[k][1], probs[k][2], nspecial)) {
            fprintf(stderr, "FAILED: L %d whole-word %d probabilities %d nspecial %d\n", L, ww, k, nspecial); return 1;
        }
        ++cases;
    }
    printf("mlm ok: %lld cases\n", (long long)cases);
    return 0;
}
#endif
