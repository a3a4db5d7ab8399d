// bf_denoisetest.cpp -- TEST-ONLY: the lane code of the span-corruption call (blingfire_amd/csrc/bf_denoise.h: the reach, the segmented max-scan with its
// chunk carry, the begin test, the run index and its cap, the running counts, the two positions) compiled for the host and driven in the lane
// partition of k_rows_denoise: G lanes per row, the row walked once in chunks of G cells with the carries, then the tails, the eos, the counts and
// the status bit.  A shuffle is an index into the chunk's arrays here, a ballot a loop over the group's lanes.  With BF_DENOISETEST_MAIN the file is
// a program of its own over exactly sized heap arrays (tests build it with -fsanitize=address,undefined).
#include <stdint.h>
#include <stddef.h>
#include <vector>
#include "../../blingfire_amd/csrc/bf_rows.h"
#include "../../blingfire_amd/csrc/bf_denoise.h"

using namespace bfa;

extern "C" {

// denoise_spec alone: 1 = accepted, 0 = refused
int bft_denoise_spec_ok(int nspecial, const int32_t *special_ids, double start_prob, int len_lo, int len_hi, int sentinel_first, int sentinel_step, int max_sentinels)
{
    DenoiseSpec sp;
    return denoise_spec(nspecial, special_ids, start_prob, len_lo, len_hi, sentinel_first, sentinel_step, max_sentinels, 1, 0, -100, 1, 0, &sp) ? 1 : 0;
}

// k_rows_denoise over nrows rows with `group` lanes per row (0 = span_group(row_len)); row_base is added to the row index the generator sees.  The
// arguments and the refusals of RowsDenoiseBatchDevice (no handle); any output may be NULL.  *status_out (may be NULL) gets the status word.
// Returns 0, or -1 = refused.
int bft_denoise_rows(const int32_t *rows, int row_len, int64_t nrows, int64_t row_base, const uint8_t *mask, const int32_t *seg, int nspecial, const int32_t *special_ids,
                     double start_prob, int len_lo, int len_hi, int sentinel_first, int sentinel_step, int max_sentinels, int eos_id, int pad_id, int ignore_label,
                     uint64_t seed, uint32_t epoch, int enc_len, int32_t *enc, int32_t *enc_cell, int32_t *enc_count, int dec_len, int32_t *dec, int32_t *dec_cell,
                     int32_t *dec_count, int32_t *span_count, int group, int *status_out)
{
    DenoiseSpec sp;
    const bool want_enc = enc || enc_cell, want_dec = dec || dec_cell;
    if (row_len < 1 || row_len > DENOISE_MAX_LEN || nrows < 0 || group < 0 || group > 64 || (group & (group - 1))) return -1;
    if ((want_enc && (enc_len < 1 || enc_len > DENOISE_MAX_LEN)) || (want_dec && (dec_len < 1 || dec_len > DENOISE_MAX_LEN))) return -1;
    if (!denoise_spec(nspecial, special_ids, start_prob, len_lo, len_hi, sentinel_first, sentinel_step, max_sentinels, eos_id, pad_id, ignore_label, seed, epoch, &sp)) return -1;
    if (nrows > 0 && (!rows || !(want_enc || want_dec || enc_count || dec_count || span_count))) return -1;
    if (!want_enc) enc_len = 0;
    if (!want_dec) dec_len = 0;
    const int G = group > 0 ? group : span_group(row_len);
    int status = 0;
    std::vector<int32_t> id((size_t)G);
    std::vector<uint8_t> present((size_t)G), eligible((size_t)G), noise0((size_t)G);
    std::vector<DenoiseScan> sc((size_t)G), next((size_t)G);
    std::vector<int> v((size_t)G);
    for (int64_t r = 0; r < nrows; ++r) {
        const int64_t base = r * row_len, ebase = r * (int64_t)enc_len, dbase = r * (int64_t)dec_len;
        DenoiseCarry carry = denoise_carry_none();
        for (int j0 = 0; j0 < row_len; j0 += G) {
            for (int l = 0; l < G; ++l) {
                const int j = j0 + l;
                id[(size_t)l] = 0; present[(size_t)l] = 0; eligible[(size_t)l] = 0;
                if (j < row_len) {
                    const uint8_t mb = mask ? mask[base + j] : (uint8_t)1;
                    const int32_t sg = seg ? seg[base + j] : 1;
                    id[(size_t)l] = rows[base + j];
                    present[(size_t)l] = denoise_present(mb, sg);
                    eligible[(size_t)l] = mlm_eligible(sp.m, id[(size_t)l], mb, sg);
                }
                const int reach = eligible[(size_t)l] ? denoise_reach(sp, mlm_draw(sp.m, r + row_base, j), j) : 0;
                sc[(size_t)l] = denoise_scan_seed(eligible[(size_t)l] != 0, reach);
            }
            for (int d = 1; d < G; d <<= 1) {
                for (int l = 0; l < G; ++l)         // (the element crosses the lanes packed into one word, as in the kernel)
                    next[(size_t)l] = denoise_scan_step(sc[(size_t)l], denoise_scan_unpack(denoise_scan_pack(sc[(size_t)(l >= d ? l - d : l)])), l >= d);
                sc = next;
            }
            uint64_t begin0_lanes = 0, noise_lanes = 0, keep_lanes = 0;
            for (int l = 0; l < G; ++l) {
                v[(size_t)l] = denoise_scan_close(sc[(size_t)l], carry.reach);
                noise0[(size_t)l] = denoise_noise0(v[(size_t)l], j0 + l);
            }
            for (int l = 0; l < G; ++l)
                if (denoise_begin0(noise0[(size_t)l] != 0, (l ? noise0[(size_t)l - 1] : carry.noise0) != 0)) begin0_lanes |= (uint64_t)1 << l;
            for (int l = 0; l < G; ++l) {
                const bool noise = denoise_noise(sp, noise0[(size_t)l] != 0, denoise_run_index(carry, begin0_lanes, l));
                if (noise) noise_lanes |= (uint64_t)1 << l;
                if (present[(size_t)l] && !noise) keep_lanes |= (uint64_t)1 << l;
            }
            const uint64_t begin_lanes = begin0_lanes & noise_lanes;
            for (int l = 0; l < G; ++l) {
                const int j = j0 + l, run = denoise_run_index(carry, begin0_lanes, l);
                const bool noise = ((noise_lanes >> l) & 1) != 0, keep = ((keep_lanes >> l) & 1) != 0, begin = ((begin_lanes >> l) & 1) != 0;
                const DenoiseSlots n = denoise_slots(carry, keep_lanes, noise_lanes, begin_lanes, l);
                if (keep || begin) {
                    const int e = denoise_enc_pos(n);
                    if (e < enc_len) {
                        if (enc) enc[ebase + e] = keep ? id[(size_t)l] : denoise_sentinel(sp, run);
                        if (enc_cell) enc_cell[ebase + e] = keep ? j : -1;
                    }
                }
                if (begin) {
                    const int d = denoise_dec_sentinel_pos(n);
                    if (d < dec_len) {
                        if (dec) dec[dbase + d] = denoise_sentinel(sp, run);
                        if (dec_cell) dec_cell[dbase + d] = -1;
                    }
                }
                if (noise) {
                    const int d = denoise_dec_pos(n, begin);
                    if (d < dec_len) {
                        if (dec) dec[dbase + d] = id[(size_t)l];
                        if (dec_cell) dec_cell[dbase + d] = j;
                    }
                }
            }
            carry = denoise_carry_next(carry, v[(size_t)G - 1], j0 + G - 1, begin0_lanes, keep_lanes, noise_lanes, begin_lanes);
        }
        const int ne = denoise_enc_count(carry), nd = denoise_dec_count(sp, carry);
        for (int k = ne; k < enc_len; ++k) {
            if (enc) enc[ebase + k] = sp.pad_id;
            if (enc_cell) enc_cell[ebase + k] = -1;
        }
        for (int k = nd; k < dec_len; ++k) {
            if (dec) dec[dbase + k] = sp.ignore_label;
            if (dec_cell) dec_cell[dbase + k] = -1;
        }
        if (sp.eos_id >= 0 && nd - 1 < dec_len) {
            if (dec) dec[dbase + nd - 1] = sp.eos_id;
            if (dec_cell) dec_cell[dbase + nd - 1] = -1;
        }
        if (enc_count) enc_count[r] = ne;
        if (dec_count) dec_count[r] = nd;
        if (span_count) span_count[r] = carry.begins;
        if ((want_enc && ne > enc_len) || (want_dec && nd > dec_len)) status |= 1;
    }
    if (status_out) *status_out = status;
    return 0;
}

} // extern "C"

#ifdef BF_DENOISETEST_MAIN
#include <cstdio>

// Exactly sized heap arrays (a read or a write past them is the sanitizer's to find), every group size.  Checked here: only what needs no second
// implementation -- every group size gives what one lane per row gives; the counts bound the rows; the cell planes index the ids beside them; the
// kept cells and the noise cells, merged back by cell, are the present cells in order; truncated outputs are prefixes of the full ones and set
// the status bit exactly where a row is longer.
struct Out {
    std::vector<int32_t> enc, ecell, ecnt, dec, dcell, dcnt, spans;
    int status;
    Out(int64_t R, int el, int dl) : enc((size_t)(R * el)), ecell((size_t)(R * el)), ecnt((size_t)R), dec((size_t)(R * dl)), dcell((size_t)(R * dl)), dcnt((size_t)R), spans((size_t)R), status(0) {}
    bool operator==(const Out &o) const { return enc == o.enc && ecell == o.ecell && ecnt == o.ecnt && dec == o.dec && dcell == o.dcell && dcnt == o.dcnt && spans == o.spans && status == o.status; }
};

static int run_case(int L, int64_t R, double prob, int len_lo, int len_hi, int max_sentinels, int eos_id)
{
    const size_t n = (size_t)(R * L);
    std::vector<int32_t> rows(n), seg(n);
    std::vector<uint8_t> mask(n);
    const int32_t specials[3] = {1, 0, 102};
    uint32_t x = 99u + (uint32_t)L * 7919u + (uint32_t)len_hi * 31u + (uint32_t)max_sentinels;
    auto rnd = [&x]() { x = x * 1664525u + 1013904223u; return x >> 8; };
    for (size_t c = 0; c < n; ++c) {
        rows[c] = rnd() % 12 == 0 ? specials[rnd() % 3] : 1000 + (int32_t)(rnd() % 29000);
        mask[c] = rnd() % 10 != 0; seg[c] = (int32_t)(rnd() % 5);
    }
    auto call = [&](Out &o, int el, int dl, int g) {
        return bft_denoise_rows(rows.data(), L, R, ((int64_t)1 << 33) + 5, mask.data(), seg.data(), 3, specials, prob, len_lo, len_hi, 32099, -1, max_sentinels, eos_id, 0, -100,
                                0x123456789abcdefull, 3, el, o.enc.data(), o.ecell.data(), o.ecnt.data(), dl, o.dec.data(), o.dcell.data(), o.dcnt.data(), o.spans.data(), g, &o.status);
    };
    const int EL = L, DL = L + 2;
    Out one(R, EL, DL);
    if (call(one, EL, DL, 1) != 0 || one.status != 0) return 1;
    for (int g = 0; g <= 64; g = g ? g * 2 : 1) {
        Out o(R, EL, DL);
        if (call(o, EL, DL, g) != 0 || !(o == one)) return 1;
        std::vector<int32_t> only((size_t)R);                     // one output alone
        if (bft_denoise_rows(rows.data(), L, R, ((int64_t)1 << 33) + 5, mask.data(), seg.data(), 3, specials, prob, len_lo, len_hi, 32099, -1, max_sentinels, eos_id, 0, -100,
                             0x123456789abcdefull, 3, 0, nullptr, nullptr, nullptr, 0, nullptr, nullptr, only.data(), nullptr, g, nullptr) != 0 || only != one.dcnt) return 1;
    }
    int most_e = 0, most_d = 0;
    for (int64_t r = 0; r < R; ++r) {
        const int ne = one.ecnt[(size_t)r], nd = one.dcnt[(size_t)r], ns = one.spans[(size_t)r];
        if (ne < 0 || ne > EL || nd < (eos_id >= 0) || nd > DL || ns < 0 || ns > max_sentinels) return 1;
        most_e = ne > most_e ? ne : most_e; most_d = nd > most_d ? nd : most_d;
        std::vector<int> seen((size_t)L, 0);
        int sent_e = 0, sent_d = 0, last = -1;
        for (int k = 0; k < EL; ++k) {
            const int32_t c = one.ecell[(size_t)(r * EL + k)], id = one.enc[(size_t)(r * EL + k)];
            if (k >= ne) { if (c != -1 || id != 0) return 1; continue; }
            if (c < 0) { if (id != 32099 - sent_e) return 1; ++sent_e; continue; }
            if (c >= L || c <= last || id != rows[(size_t)(r * L + c)]) return 1;
            last = c; seen[(size_t)c] += 1;
        }
        last = -1;
        for (int k = 0; k < DL; ++k) {
            const int32_t c = one.dcell[(size_t)(r * DL + k)], id = one.dec[(size_t)(r * DL + k)];
            if (k >= nd) { if (c != -1 || id != -100) return 1; continue; }
            if (eos_id >= 0 && k == nd - 1) { if (c != -1 || id != eos_id) return 1; continue; }
            if (c < 0) { if (id != 32099 - sent_d) return 1; ++sent_d; continue; }
            if (c >= L || c <= last || id != rows[(size_t)(r * L + c)]) return 1;
            last = c; seen[(size_t)c] += 1;
        }
        if (sent_e != ns || sent_d != ns) return 1;
        for (int j = 0; j < L; ++j) if (seen[(size_t)j] != (mask[(size_t)(r * L + j)] != 0 && seg[(size_t)(r * L + j)] != 0 ? 1 : 0)) return 1;
    }
    for (int cut = 0; cut <= 1; ++cut) {                      // exactly at the longest row: nothing lost; one below: a prefix and the bit
        const int el = most_e - cut, dl = most_d - cut;
        if (el < 1 || dl < 1) continue;
        Out t(R, el, dl);
        if (call(t, el, dl, 0) != 0 || t.status != cut || t.ecnt != one.ecnt || t.dcnt != one.dcnt) return 1;
        for (int64_t r = 0; r < R; ++r) {
            for (int k = 0; k < el; ++k) if (t.enc[(size_t)(r * el + k)] != one.enc[(size_t)(r * EL + k)] || t.ecell[(size_t)(r * el + k)] != one.ecell[(size_t)(r * EL + k)]) return 1;
            for (int k = 0; k < dl; ++k) if (t.dec[(size_t)(r * dl + k)] != one.dec[(size_t)(r * DL + k)] || t.dcell[(size_t)(r * dl + k)] != one.dcell[(size_t)(r * DL + k)]) return 1;
        }
    }
    return 0;
}

int main()
{
    const int Ls[12] = {1, 2, 3, 5, 9, 31, 32, 33, 64, 65, 129, 200};
    int64_t cases = 0;
    for (int L : Ls)
        for (double prob : {0.0, 0.08, 0.5, 1.0})
            for (int hi : {1, 5, L + 3})
                for (int cap : {1, 2, 100}) {
                    const int lo = hi == 5 ? 2 : 1, eos = cap == 2 ? -1 : 1;
                    if (run_case(L, 9, prob, lo, hi, cap, eos)) { fprintf(stderr, "FAILED: L %d prob %g len %d..%d cap %d\n", L, prob, lo, hi, cap); return 1; }
                    ++cases;
                }
    printf("denoise ok: %lld cases\n", (long long)cases);
    return 0;
}
#endif
