// bf_w2htest.cpp -- TEST-ONLY: the hyphenator's lane programs (blingfire_amd/csrc/bf_w2h.h) compiled for the host and driven sequentially,
// the way bf_kernels_w2h.hip drives them on the device: prep per word into the position stream, one walk per (word, From) into a byte of
// seen values per slot, the flags written over the classes, sizes, a scan, the copy with its capacity guard.
#include <cstring>
#include <vector>
#include "hosttest.h"
#include "ws_sizes.h"
#include "../../blingfire_amd/csrc/bf_w2h.h"

using namespace bfa;

static W2hTables tables_of(const Model &m)
{
    W2hTables t;
    t.T = m.w2h.t64.data(); t.pats = m.w2h_pats.data(); t.cp_l1 = m.w2h_cpmap.l1.data(); t.cp_pages = m.w2h_cpmap.pages.data();
    t.initial = m.w2h.initial_base; t.cls_l = m.w2h_cls_l; t.cls_r = m.w2h_cls_r; t.min_pat_len = m.w2h_min_pat_len; t.no_hyph_len = m.w2h_no_hyph_len;
    return t;
}

extern "C" {

int bft_w2h_ready(void *hv) { return ((Handle *)hv)->m.w2h_ready ? 1 : 0; }
int bft_w2h_facts(void *hv, int *out)      // has, ready, ignore-case, min-len, min-len2, left anchor, right anchor, classes, table entries, pattern bytes
{
    const Model &m = ((Handle *)hv)->m;
    const int v[10] = {m.has_w2h, m.w2h_ready, m.w2h_ignore_case, m.w2h_min_pat_len, m.w2h_no_hyph_len, m.w2h_left_anchor, m.w2h_right_anchor, m.w2h.nclasses,
                       (int)m.w2h.t64.size(), (int)m.w2h_pats.size()};
    memcpy(out, v, sizeof v);
    return 10;
}

// WordHyphenationBatch: returns the byte total (offsets complete); bytes at or past cap are not written.  -5: no usable [w2h], -1: a uHy that cannot be encoded
long long bft_w2h_batch(void *hv, const unsigned char *text, const long long *off, long long n, int u_hy, unsigned char *out, long long cap, long long *out_off)
{
    const Model &m = ((Handle *)hv)->m;
    if (!m.w2h_ready) return -5;
    uint32_t hy_bytes = 0; const int hy_len = w2h_encode(u_hy, &hy_bytes);
    if (hy_len == 0) return -1;
    const W2hTables t = tables_of(m);
    const long long total = n > 0 ? off[n] : 0;
    std::vector<uint16_t> cls((size_t)ws_w2h_cells(n, total), 0xDEAD);      // ws_sizes.h: what the product reserves
    std::vector<int> nch((size_t)n + 1), srcb((size_t)n + 1), lens((size_t)n + 1);
    for (long long w = 0; w < n; ++w) {
        if (off[w] < 0 || off[w + 1] < off[w] || off[w + 1] > total) { nch[(size_t)w] = srcb[(size_t)w] = 0; continue; }
        nch[(size_t)w] = w2h_prep_word(t, text + off[w], off[w + 1] - off[w], cls.data() + w2h_slot(off[w], w), &srcb[(size_t)w]);
    }
    std::vector<uint8_t> seen;
    for (long long w = 0; w < n; ++w) {
        const int c = nch[(size_t)w];
        uint16_t *wc = cls.data() + w2h_slot(off[w], w);
        seen.assign((size_t)c + 1, 0);
        for (int from = 0; from < c + 2; ++from)
            if (w2h_starts_at(t, c, from)) w2h_walk(t, wc, c, from, [&](int slot, int v) { seen.at((size_t)slot) |= (uint8_t)(1u << v); });
        int nhy = 0;
        for (int i = 0; i < c; ++i) { const bool hy = w2h_hyphen_after(t, seen[(size_t)i], i, c); wc[1 + i] = hy ? 1 : 0; nhy += hy; }
        lens[(size_t)w] = c > 0 ? srcb[(size_t)w] + nhy * hy_len : 0;
    }
    out_off[0] = 0;
    for (long long w = 0; w < n; ++w) out_off[w + 1] = out_off[w] + lens[(size_t)w];
    for (long long w = 0; w < n && out; ++w) {
        if (nch[(size_t)w] <= 0) continue;
        const unsigned char *s = text + off[w]; const long long len = off[w + 1] - off[w];
        if (len >= 3 && s[0] == 0xEF && s[1] == 0xBB && s[2] == 0xBF) s += 3;
        w2h_copy_word(s, nch[(size_t)w], cls.data() + w2h_slot(off[w], w) + 1, hy_bytes, hy_len, [&](int o, uint8_t c) { if (out_off[w] + o < cap) out[out_off[w] + o] = c; });
    }
    return out_off[n];
}

// WordHyphenationWithModel as bf_capi.cpp assembles it from a batch of one
int bft_w2h_one(void *hv, const char *s, int n, char *out, int cap, int u_hy)
{
    const Model &m = ((Handle *)hv)->m;
    if (n == 0) return 0;
    if (n < 0 || n > 1000000000 || !s || !m.w2h_ready) return -1;
    const long long up = n < 3 + 4 * W2H_MAX_CHARS ? n : 3 + 4 * W2H_MAX_CHARS, off[2] = {0, up};
    long long out_off[2] = {0, 0};
    unsigned char full[8 * W2H_MAX_CHARS + 16];
    const long long r = bft_w2h_batch(hv, (const unsigned char *)s, off, 1, u_hy, full, (long long)sizeof full, out_off);
    if (r <= 0) return -1;
    return w2h_finish(full, (int)r, out, cap);
}

} // extern "C"
