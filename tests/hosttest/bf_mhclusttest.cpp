// Host emulation of MinHashClustersBatchDevice (bf_kernels_mhclust.hip): the lane code of blingfire_amd/csrc/bf_mhclust.h -- slot choice, probing
// with the side slot, find and unite -- run lane after lane under the sequential memory policy, in the kernels' order: per band clear, insert,
// link; then flatten and sizes.  `reverse` visits the sequences of every pass from the last to the first: the slots differ, the outputs may not.
// With BF_MHCLUSTTEST_MAIN the file is a program of its own over exactly sized heap arrays (tests build it with -fsanitize=address,undefined).
#include <stddef.h>
#include <stdint.h>
#include <vector>
#include "../../blingfire_amd/csrc/bf_mhclust.h"

using namespace bfa;

extern "C" {

// {the empty mark (as int64), slots of a table for nseq = 1000, the home slot of key 0 there}
void bft_mhclust_geometry(int64_t *out)
{
    out[0] = (int64_t)MHC_EMPTY; out[1] = mhclust_slots(1000); out[2] = mhclust_home(0, mhclust_slots(1000) - 1);
}

// returns 0, -1 for refused parameters.  keep and size may be NULL.  info[0] = the longest probe sequence of an insert, in slots.
int bft_mhclust_batch(const int32_t *sig, int H, const int64_t *keys, int B, int64_t nseq, const int32_t *nshingles, int min_equal, int reverse, int32_t *label,
                      uint8_t *keep, int32_t *size, int64_t *counts, int64_t *info)
{
    if (!mhclust_spec(H, B, nseq, min_equal, 0) || !counts || (nseq > 0 && (!keys || !label || (min_equal > 0 && !sig)))) return -1;
    const int64_t T = mhclust_slots(nseq);
    std::vector<uint64_t> tkey((size_t)T);
    std::vector<int32_t> trep((size_t)T), sizes((size_t)nseq, 0);
    counts[0] = counts[1] = 0; info[0] = 0;
    for (int64_t q = 0; q < nseq; ++q) label[q] = (int32_t)q;
    auto at = [&](int64_t i) { return reverse ? nseq - 1 - i : i; };
    for (int band = 0; band < B; ++band) {
        for (int64_t i = 0; i < T; ++i) { tkey[(size_t)i] = MHC_EMPTY; trep[(size_t)i] = MHC_NONE; }
        for (int64_t i = 0; i < nseq; ++i) {
            const int64_t q = at(i);
            if (mhclust_live(nshingles, q)) mhclust_insert<MhcSeq>(tkey.data(), trep.data(), T, (uint64_t)keys[q * B + band], (int32_t)q);
        }
        for (int64_t s = 0, run = 0; s < 2 * (T - 1); ++s) {                    // the longest run of taken slots, around the end of the table too
            run = tkey[(size_t)(s % (T - 1))] != MHC_EMPTY ? run + 1 : 0;
            if (run > info[0]) info[0] = run < T - 1 ? run : T - 1;
        }
        for (int64_t i = 0; i < nseq; ++i) {
            const int64_t q = at(i);
            if (!mhclust_live(nshingles, q)) continue;
            const int32_t f = mhclust_lookup(tkey.data(), trep.data(), T, (uint64_t)keys[q * B + band]);
            if (f > (int32_t)q) return -2;                                      // a live sequence finds itself or a smaller one
            if (f == (int32_t)q) continue;
            ++counts[1];
            int cnt = 0;
            for (int k = 0; min_equal > 0 && k < H; ++k) cnt += sig[q * H + k] == sig[(int64_t)f * H + k];
            if (cnt >= min_equal) mhclust_unite<MhcSeq>(label, (int32_t)q, f);
        }
    }
    for (int64_t i = 0; i < nseq; ++i) {
        const int64_t q = at(i);
        const int32_t r = mhclust_find<MhcSeq>(label, (int32_t)q);
        label[q] = r;
        if (keep) keep[q] = r == (int32_t)q;
        ++sizes[(size_t)r];
        counts[0] += r == (int32_t)q;
    }
    for (int64_t q = 0; size && q < nseq; ++q) size[q] = sizes[(size_t)label[q]];
    return 0;
}

} // extern "C"

#ifdef BF_MHCLUSTTEST_MAIN
#include <cstdio>

// Exactly sized heap arrays (a read or a write past them is the sanitizer's to find).  Checked here: only what needs no second implementation --
// the named shapes have components known by construction, and visiting the sequences in reverse gives the same bytes.
namespace {

struct Out { std::vector<int32_t> label, size; std::vector<uint8_t> keep; int64_t counts[2], info[1]; };

int run(const std::vector<int64_t> &keys, int B, int64_t nseq, const std::vector<int32_t> &sig, int H, const std::vector<int32_t> &nsh, int min_equal, Out *o)
{
    Out r[2];
    for (int rev = 0; rev < 2; ++rev) {
        r[rev].label.assign((size_t)nseq, -7); r[rev].size.assign((size_t)nseq, -7); r[rev].keep.assign((size_t)nseq, 7);
        if (bft_mhclust_batch(sig.empty() ? nullptr : sig.data(), H, keys.data(), B, nseq, nsh.empty() ? nullptr : nsh.data(), min_equal, rev, r[rev].label.data(),
                              r[rev].keep.data(), r[rev].size.data(), r[rev].counts, r[rev].info) != 0) return 1;
    }
    if (r[0].label != r[1].label || r[0].size != r[1].size || r[0].keep != r[1].keep || r[0].counts[0] != r[1].counts[0] || r[0].counts[1] != r[1].counts[1]) return 2;
    *o = r[0];
    return 0;
}

bool one_cluster(const Out &o, int64_t nseq)
{
    for (int64_t q = 0; q < nseq; ++q) if (o.label[(size_t)q] != 0 || o.size[(size_t)q] != nseq || o.keep[(size_t)q] != (q == 0)) return false;
    return o.counts[0] == 1;
}

int shapes()
{
    const int64_t n = 5000;
    const std::vector<int32_t> none;
    Out o;
    for (int B : {1, 3}) {                                                      // all keys equal: one slot, one cluster, every other sequence a candidate per band
        std::vector<int64_t> k((size_t)(n * B), 42);
        if (run(k, B, n, none, 1, none, 0, &o) || !one_cluster(o, n) || o.counts[1] != (n - 1) * B || o.info[0] != 1) return 10 + B;
    }
    {                                                                           // all keys distinct: no candidate; probes stay short in a table half full
        std::vector<int64_t> k((size_t)(n * 2));
        for (size_t i = 0; i < k.size(); ++i) k[i] = (int64_t)i * 7919;
        if (run(k, 2, n, none, 1, none, 0, &o) || o.counts[0] != n || o.counts[1] != 0 || o.info[0] > 128) return 20;
        for (int64_t q = 0; q < n; ++q) if (o.label[(size_t)q] != q || o.size[(size_t)q] != 1 || !o.keep[(size_t)q]) return 21;
    }
    for (int rev = 0; rev < 2; ++rev) {                                         // a chain: q and q + 1 share exactly band q % B; reversed: the indices mirrored
        const int B = 5;
        std::vector<int64_t> k((size_t)(n * B));
        for (int64_t q = 0; q < n; ++q) for (int b = 0; b < B; ++b) k[(size_t)(q * B + b)] = (q + 1) * 1000 + b;
        for (int64_t q = 0; q + 1 < n; ++q) {
            const int64_t x = rev ? n - 1 - q : q, y = rev ? x - 1 : x + 1;
            k[(size_t)(y * B + q % B)] = k[(size_t)(x * B + q % B)];
        }
        if (run(k, B, n, none, 1, none, 0, &o) || !one_cluster(o, n) || o.counts[1] != n - 1) return 30 + rev;
    }
    {                                                                           // 0, -1, INT64_MIN and the empty mark, each twice, one band; sequence 8 not live
        const int64_t v[4] = {0, -1, INT64_MIN, (int64_t)MHC_EMPTY};
        std::vector<int64_t> k = {v[0], v[1], v[2], v[3], v[0], v[1], v[2], v[3], v[3], 5};
        std::vector<int32_t> nsh(10, 1);
        nsh[8] = 0;
        if (run(k, 1, 10, none, 1, nsh, 0, &o) || o.counts[0] != 6 || o.counts[1] != 4) return 40;
        for (int q = 0; q < 8; ++q) if (o.label[(size_t)q] != q % 4 || o.size[(size_t)q] != 2) return 41;
        if (o.label[8] != 8 || o.label[9] != 9 || o.size[8] != 1) return 42;
    }
    {                                                                           // verified links: 1 passes against 0, 2 does not; 2 and 1 would pass each other
        const int H = 4;
        std::vector<int64_t> k = {9, 9, 9};
        std::vector<int32_t> sig = {1, 1, 1, 1, 1, 1, 0, 0, 0, 1, 0, 0};
        if (run(k, 1, 3, sig, H, none, 2, &o) || o.counts[0] != 2 || o.counts[1] != 2 || o.label[1] != 0 || o.label[2] != 2) return 50;
        if (run(k, 1, 3, sig, H, none, 1, &o) || o.counts[0] != 1) return 51;
    }
    int64_t counts[2] = {-1, -1}, info[1];
    if (bft_mhclust_batch(nullptr, 1, nullptr, 1, 0, nullptr, 0, 0, nullptr, nullptr, nullptr, counts, info) != 0 || counts[0] != 0 || counts[1] != 0) return 60;
    if (bft_mhclust_batch(nullptr, 1, nullptr, 257, 0, nullptr, 0, 0, nullptr, nullptr, nullptr, counts, info) != -1) return 61;
    // range reduction: the home of every key is a regular slot, for table sizes that are no power of two
    for (int64_t R : {(int64_t)63, (int64_t)65, (int64_t)10063, ((int64_t)1 << 32) + 61})
        for (uint64_t key : {(uint64_t)0, (uint64_t)1, ~(uint64_t)0, (uint64_t)1 << 63, MHC_EMPTY - 1}) {
            const int64_t s = mhclust_home(key, R);
            if (s < 0 || s >= R) return 70;
        }
    if (mhclust_mulhi(~0ull, ~0ull) != ~0ull - 1 || mhclust_mulhi(1ull << 63, 6) != 3 || mhclust_mulhi(0x123456789ABCDEF0ull, 1ull << 32) != 0x12345678ull) return 71;
    return 0;
}

} // namespace

int main()
{
    const int r = shapes();
    if (r != 0) { printf("mhclust FAILED: %d\n", r); return 1; }
    printf("mhclust ok: named shapes, both visiting orders\n");
    return 0;
}
#endif
