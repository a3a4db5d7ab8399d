// Host emulation of IdsToNgramSetBatchDevice / IdsNgramOverlapBatchDevice (bf_kernels_ngram.hip): the lane code of blingfire_amd/csrc/bf_ngram.h run
// lane after lane under the sequential memory policy, in the kernel's partition and order -- tiles of 1,024 positions, 16 positions a lane, the
// staged halos in the skewed block, Horner and roll, the probes, the bitmap window, the run counts.  With BF_NGRAMTEST_MAIN the file is a program
// of its own over exactly sized heap arrays (tests build it with -fsanitize=address,undefined).
#include <stddef.h>
#include <stdint.h>
#include <vector>
#include "../../blingfire_amd/csrc/bf_ngram.h"

using namespace bfa;

extern "C" {

// mode 0 = the overlap call, 1 = the set call adding to the table, 3 = the set call clearing it first.  Returns the status word, -1 when refused.
int bft_ngram_batch(const int32_t *ids, int64_t ids_len, const int64_t *off, int64_t nseq, int n, uint64_t seed, int mode, uint64_t *table, int64_t slots,
                    int64_t *counts, int32_t *ngrams, int32_t *hits, int32_t *covered, uint8_t *mask)
{
    if (!ngram_spec(n, slots, nseq, ids_len) || !table || !off) return -1;
    const bool set = mode != 0;
    int status = 0;
    std::vector<int64_t> W((size_t)nseq + 1, 0);
    for (int64_t q = 0; q < nseq; ++q) {
        bool bad;
        const int32_t len = minhash_len(off[q], off[q + 1], ids_len, &bad);
        if (bad) status |= 8;
        if (ngrams) ngrams[q] = ngram_count(len, n);
        W[(size_t)q + 1] = W[(size_t)q] + len;
    }
    if (set) { counts[0] = counts[1] = counts[2] = 0; for (int64_t i = 0; (mode & 2) && i < slots; ++i) table[i] = 0; }
    for (int64_t q = 0; q < nseq; ++q) if (!ngram_inside(W[(size_t)q], W[(size_t)q + 1])) { if (hits) hits[q] = 0; if (covered) covered[q] = 0; }
    const int64_t T = W[(size_t)nseq];
    std::vector<uint64_t> sm(NGRAM_STAGE_QWORDS), bm(NGRAM_BM_WORDS);
    for (int64_t tile = 0; tile < ngram_ntiles(T); ++tile) {
        NgramTile tl{tile * NGRAM_TILE, 0, T, n, seed, ngram_pow(n)};
        tl.t1 = tl.t0 + NGRAM_TILE < T ? tl.t0 + NGRAM_TILE : T;
        const StreamGlobal src{W.data(), off, stream_find_unit(W.data(), 0, nseq, set ? tl.t0 : ngram_stage_lo(tl.t0, n)),
                               stream_find_unit(W.data(), 0, nseq, ngram_stage_hi(tl.t1, T, n) - 1), 0};
        StreamUnit first[64];
        uint32_t vmask[64], hmask[64] = {0};
        bool left[64];
        bm.assign(bm.size(), 0);
        for (int l = 0; l < 64; ++l) {
            ngram_stage_own(tl, src, ids, l, sm.data(), &first[l], &vmask[l]);
            const int64_t tr = ngram_right_pos(tl, l), tq = set ? -1 : ngram_left_pos(tl, l);
            if (tr >= 0) ngram_stage_at(tl, src, ids, tr, ngram_pos_cell(tl, tr), sm.data());
            left[l] = tq >= 0 && ngram_stage_at(tl, src, ids, tq, ngram_pos_cell(tl, tq), sm.data());
        }
        for (int l = 0; l < 64; ++l) {
            uint64_t g[NGRAM_LANE];
            if (vmask[l]) ngram_prints(tl, sm.data(), l, vmask[l], g);
            for (int k = 0; set && vmask[l] && k < NGRAM_LANE; ++k) {
                if (!g[k]) continue;
                const int r = ngram_insert<NgramSeq>(table, slots, g[k]);
                ++counts[0]; counts[1] += r == NGRAM_STORED; counts[2] += r == NGRAM_NO_SLOT;
            }
            if (!set && vmask[l]) ngram_put_hits<NgramSeq>(bm.data(), l, hmask[l] = ngram_probe16(table, slots, g));
            const int64_t tq = ngram_left_pos(tl, l);
            if (!set && left[l] && ngram_lookup(table, slots, ngram_final(ngram_horner(sm.data(), ngram_pos_cell(tl, tq), n), n))) ngram_put_left<NgramSeq>(tl, bm.data(), tq);
        }
        for (int l = 0; !set && l < 64; ++l) ngram_runs<NgramSeq>(tl, src, first[l], l, bm.data(), hmask[l], hits, covered, mask);
    }
    return status | ((set && counts[2]) ? NGRAM_STATUS_FULL : 0);
}

// 0 = the three facts no batch reaches hold: the roll equals Horner for every n, fingerprint 0 is read as 1, a full table ends insert and look-up
int bft_ngram_facts(void)
{
    std::vector<uint64_t> sm(NGRAM_STAGE_QWORDS);
    for (size_t i = 0; i < sm.size(); ++i) sm[i] = minhash_fmix64(i + 1);
    for (int n = 1; n <= NGRAM_MAX; ++n) {
        uint64_t P = ngram_horner(sm.data(), 5, n);
        for (int k = 0; k < 40; ++k) {
            P = ngram_roll(P, sm[(size_t)ngram_lds(5 + k)], sm[(size_t)ngram_lds(5 + k + n)], ngram_pow(n));
            if (P != ngram_horner(sm.data(), 6 + k, n)) return 1;
        }
        if (ngram_final((uint64_t)n * 0xC2B2AE3D27D4EB4Full, n) != 1ull) return 2;
    }
    std::vector<uint64_t> full = {11, 12, 13};
    if (ngram_lookup(full.data(), 3, 99) || !ngram_lookup(full.data(), 3, 12) || ngram_insert<NgramSeq>(full.data(), 3, 99) != NGRAM_NO_SLOT) return 3;
    return ngram_insert<NgramSeq>(full.data(), 3, 13) == NGRAM_PRESENT ? 0 : 4;
}

} // extern "C"

#ifdef BF_NGRAMTEST_MAIN
#include <cstdio>

// Exactly sized heap arrays (a read or a write past them is the sanitizer's to find).  Checked here: only what needs no second implementation --
// a batch probed against its own set, in a table of one slot per id and one more, is all hits.
int main()
{
    if (bft_ngram_facts() != 0) { printf("ngram FAILED: facts %d\n", bft_ngram_facts()); return 1; }
    for (int n : {1, 2, 13, 16, 17, 64}) {
        std::vector<int64_t> off = {0};
        for (int64_t len : {0, n - 1, n, n + 1, 2500, 0, 3, 1, 1, 2, 1100 + n}) off.push_back(off.back() + len);
        std::vector<int32_t> ids((size_t)off.back());
        for (size_t i = 0; i < ids.size(); ++i) ids[i] = (int32_t)(minhash_fmix64(i * 64 + (size_t)n) % 3) - 1;
        const int64_t nseq = (int64_t)off.size() - 1;
        std::vector<uint64_t> table((size_t)off.back() + 1);
        std::vector<int32_t> ng((size_t)nseq), hits((size_t)nseq, -7), cov((size_t)nseq, -7);
        std::vector<uint8_t> mask(ids.size(), 7);
        int64_t counts[3];
        if (bft_ngram_batch(ids.data(), off.back(), off.data(), nseq, n, 7, 3, table.data(), (int64_t)table.size(), counts, nullptr, nullptr, nullptr, nullptr) != 0 ||
            bft_ngram_batch(ids.data(), off.back(), off.data(), nseq, n, 7, 0, table.data(), (int64_t)table.size(), nullptr, ng.data(), hits.data(), cov.data(), mask.data()) != 0 ||
            hits != ng || counts[2] != 0) { printf("ngram FAILED: n = %d\n", n); return 1; }
    }
    printf("ngram ok: facts, own-set batches\n");
    return 0;
}
#endif
