// bf_unioffstest.cpp -- TEST-ONLY: the offsets instance of the Unigram cut form (bf_seg.h UniCut<.., .., true>) in the host driver's trip -- K
// transitions, the end of the start position, the short way out, the emission phase, spills, and a trip limit that turns a stall into a
// failure -- then what k_uni_ids does per token: the id of the token word, (from, to) from the span words (uni_token_span), the byte offsets from
// the prologue's element -> source byte map.  Checked against
//   * the oracle's (id, first byte, last byte) on the case table below, for every Unigram model it is given, dummy prefix on and off;
//   * the sequential restatement seg_unigram_doc (itself pinned to the oracle) on a three-entry dictionary with a positive score, where the
//     backward pass lands on a position without incoming arc: the restart, which no shipped model reaches.
// bft_unioffs_run returns the number of differences and counts how often the restart, a spill and the short way out were taken.
// With -DBF_UNIOFFS_MAIN the unit is a stand-alone program (bf_unioffs MODEL...), built under the address and undefined-behaviour sanitizers
// by blingfire_amd/build.py build_unioffs_san(); it is never loaded into python in that form.
#include "hosttest.h"
#include "../../blingfire_amd/csrc/bf_seg.h"
#include "../../oracle/bf_oracle.h"

#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

using namespace bfa;

namespace {

struct CutRing {
    std::vector<double> v; std::vector<uint8_t> r; int smask, rmask;
    double score(int pos) const { return v[(size_t)(pos & smask)]; }
    uint32_t rec(int pos) const { return r[(size_t)(pos & rmask)]; }
    void set(int pos, double x, uint32_t rr) { v[(size_t)(pos & smask)] = x; r[(size_t)(pos & rmask)] = (uint8_t)rr; }
    void setrec(int pos, uint32_t rr) { r[(size_t)(pos & rmask)] = (uint8_t)rr; }
    void setscore(int pos, double x) { v[(size_t)(pos & smask)] = x; }
    void fill(double x) { for (auto &e : v) e = x; for (auto &e : r) e = 0x5A; }      // (record slots are not initialised on the device either)
};
struct HostSeek { const uint16_t *cp; uint32_t operator()(int i) const { return cp[i]; } void seek(int) const {} void advance(int) const {} };
// token words and span words of one document, each array exactly L long; a group of four must be aligned in both (the device's two staging arrays)
struct HostPut {
    std::vector<uint32_t> &toks, &spans; int align; bool &bad;
    void operator()(int k, uint32_t v) const { toks.at((size_t)k) = v; }
    void span(int k, uint32_t v) const { spans.at((size_t)k) = v; }
    void quad(int k, uint32_t a, uint32_t b, uint32_t c, uint32_t d) const { if (((k + align) & 3) != 0) bad = true; (*this)(k, a); (*this)(k + 1, b); (*this)(k + 2, c); (*this)(k + 3, d); }
    void span_quad(int k, uint32_t a, uint32_t b, uint32_t c, uint32_t d) const { if (((k + align) & 3) != 0) bad = true; span(k, a); span(k + 1, b); span(k + 2, c); span(k + 3, d); }
};
struct Driver { int W, period, K, quick; };
const Driver DRIVERS[4] = {{32, 1, 3, 1}, {32, 32, 3, 1}, {64, 1 << 30, 1, 1}, {32, 3, 4, 0}};      // ring, emission period, transitions per trip, the short way out
enum { R_RESTART = 0, R_SPILL = 1, R_QUICK = 2 };

// One document through the offsets instance: ids[k], from[k], to[k] for k < min(tokens, max_ids).  Returns that count; -3 a write outside
// the document's own range or an unwritten place, -5 the driver stalled.
int cut_doc(const SegTables &S, const int32_t *idcol, const uint16_t *cp, int L, int depth, const Driver &dr, int align, int max_ids, int unk,
            std::vector<int32_t> &ids, std::vector<int> &from, std::vector<int> &to, unsigned long long *reached)
{
    ids.clear(); from.clear(); to.clear();
    if (L <= 0) return 0;
    int ring_n = 1; while (ring_n < depth) ring_n <<= 1;
    int W = dr.W; while (W < depth + UC_SPILL + 4) W <<= 1;
    CutRing ring{std::vector<double>((size_t)ring_n), std::vector<uint8_t>((size_t)W), ring_n - 1, W - 1};
    HostSeek hs{cp};
    UniCut<HostSeek, CutRing, true> uc(S, hs, ring);
    std::vector<uint8_t> spill_all((size_t)L + 64, (uint8_t)0xEE);
    uc.init(L, depth, W, spill_all.data() + 32);
    std::vector<uint32_t> toks((size_t)L, 0xDEADBEEFu), spans((size_t)L, 0xDEADBEEFu);
    bool bad = false;
    HostPut put{toks, spans, align, bad};
    uc.tok_align = align;
    for (unsigned long long trip = 1;; ++trip) {
        const bool can = uc.room(dr.K);
        bool done = false;
        if (can) {
            for (int u = 0; u < dr.K; ++u) if (uc.walking) uc.step();
            if (!uc.walking) done = uc.finish_start() == UC_DONE;
            if (dr.quick) { const int before = uc.nout; uc.quick(put); if (uc.nout > before) ++reached[R_QUICK]; }
        }
        if (done || !can || trip % (unsigned long long)dr.period == 0) {
            if (uc.pending()) { const int before = uc.nout; uc.emit(put); if (uc.nout <= before) ++reached[R_RESTART]; }
            else if (!can) { uc.spill(dr.K); ++reached[R_SPILL]; }
        }
        if (done) break;
        if (trip > 64ull * (unsigned long long)L + 1024ull) return -5;
    }
    if (bad || spill_all[31] != 0xEE || spill_all[(size_t)L + 32] != 0xEE) return -3;
    const int n = uc.nout < max_ids ? uc.nout : max_ids;
    for (int k = 0; k < n; ++k) {
        if (toks[(size_t)k] == 0xDEADBEEFu || spans[(size_t)k] == 0xDEADBEEFu) return -3;
        int f, t;
        uni_token_span(spans.data(), k, f, t);
        ids.push_back(uni_token_id(S, idcol, hs, toks[(size_t)k], unk)); from.push_back(f); to.push_back(t);
    }
    return n;
}

// the case table: the smallest documents at which the span words can go wrong (tests/test_gpu_unioffs.py runs the same ones on the device)
const char *const DOCS[] = {
    "", " ", "a", "\xF0\x9F\x98\x80",                                                                    // from == to; the end covers a 4-byte character
    "\xC2\xAA \xEF\xAC\x81 \xE3\x8D\xBF", "x\xEF\xAC\x81y word\xC2\xAA", "a\xE3\x8D\xBF",                  // 1:n charmap characters inside and at the end of a word
    "pneumonoultramicroscopicsilicovolcanoconi next",                                                     // a word of 40 letters: the ring spills
    "hello \xF3\xB0\x80\x80 world",                                                                       // an unknown run of one character
    "Hello, world! This is a test of unaffable.", "   hello  ",
};
std::string unknown_run() { std::string s = "a "; for (int k = 0; k < 200; ++k) s += "\xF3\xB0\x80\x80"; return s + " b"; }      // longer than UC_RUN_MAX
std::string no_blanks()                                                                                    // Thai and CJK, about 300 characters
{
    std::string s;
    for (int k = 0; k < 12; ++k) s += "\xE0\xB8\x81\xE0\xB8\xB2\xE0\xB8\xA3\xE0\xB8\x97\xE0\xB8\x94\xE0\xB8\xAA\xE0\xB8\xAD\xE0\xB8\x9A\xE0\xB8\xA0\xE0\xB8\xB2\xE0\xB8\xA9\xE0\xB8\xB2\xE0\xB9\x84\xE0\xB8\x97\xE0\xB8\xA2";
    for (int k = 0; k < 30; ++k) s += "\xE6\x97\xA5\xE6\x9C\xAC\xE8\xAA\x9E\xE3\x81\xAE\xE3\x83\x86";
    return s;
}

long model_cases(Handle &h, bfo_model *o, unsigned long long *reached)
{
    Model &m = h.m;
    SegTables S;
    S.T = m.dict.t64.data(); S.info = (const SegInfo *)m.seg_info.data(); S.initial = m.dict.initial_base; S.cls_delim = m.sp_delim_code;
    S.kind = m.kind; S.id_offset = m.id_offset; S.score = m.seg_score.data(); S.leaf_lo = m.dict.leaf_lo; S.leaf_n = m.dict.leaf_n;
    std::vector<std::string> docs(DOCS, DOCS + sizeof DOCS / sizeof DOCS[0]);
    docs.push_back(unknown_run()); docs.push_back(no_blanks());
    long diffs = 0;
    for (int nodummy = 0; nodummy < 2; ++nodummy) {
        m.no_dummy_prefix = nodummy != 0; bfo_set_no_dummy_prefix(o, nodummy);
        for (size_t d = 0; d < docs.size(); ++d) for (int mx : {4096, 3}) {
            const int n = (int)docs[d].size();
            std::vector<char> s((size_t)n + 2, 'A');          // the oracle reads the byte in front of the string for a token made of the dummy prefix alone
            if (n) memcpy(s.data() + 1, docs[d].data(), (size_t)n);
            std::vector<int32_t> wi((size_t)mx); std::vector<int> ws((size_t)mx), we((size_t)mx);
            int want = bfo_text_to_ids_with_offsets(o, s.data() + 1, n, wi.data(), ws.data(), we.data(), mx, 3);
            if (want < 0) want = 0;
            if (want > mx) want = mx;
            std::vector<uint16_t> st; std::vector<int> src_off;
            const bool ok = bft_sp_stream(m, docs[d].data(), n, st, &src_off);
            for (int k = 0; k < 4; ++k) {
                std::vector<int32_t> ids; std::vector<int> from, to;
                const int got = ok ? cut_doc(S, m.i2info_id.data(), st.data(), (int)st.size(), m.trie_max_depth, DRIVERS[k], (int)((d + (size_t)k) & 3), mx, 3, ids, from, to, reached) : 0;
                bool same = got == want;
                for (int i = 0; same && i < got; ++i) {      // what k_uni_ids makes of (from, to): k_compact's rule
                    const int so = from[(size_t)i] >= 0 ? src_off[(size_t)from[(size_t)i]] : -1, eo = src_off[(size_t)to[(size_t)i]];
                    int sz = 0;
                    if (eo >= 0) { const unsigned ch = (unsigned char)docs[d][(size_t)eo]; sz = (ch & 0x80) == 0 ? 1 : (ch & 0xE0) == 0xC0 ? 2 : (ch & 0xF0) == 0xE0 ? 3 : (ch & 0xF8) == 0xF0 ? 4 : 0; }
                    same = ids[(size_t)i] == wi[(size_t)i] && so == ws[(size_t)i] && eo + (sz > 0 ? sz - 1 : 0) == we[(size_t)i];
                }
                if (!same) { ++diffs; fprintf(stderr, "unioffs: %s document %ld max_ids %d driver %d no_dummy_prefix %d: %d tokens, the oracle %d, or other values\n", h.path.c_str(), (long)d, mx, k, nodummy, got, want); }
            }
        }
    }
    m.no_dummy_prefix = false; bfo_set_no_dummy_prefix(o, 0);
    return diffs;
}

// The restart.  Classes 0 1 2, entries "01" (-3e38), "1" (+3e38), "2" (-3e38): in "2201" the arc "1" from position 3 beats "01" although position 2 has
// no incoming arc, so the backward pass lands there, emits <UnkId, -1, 2> and stops -- "22" is dropped (..._1best_t.h:250-262).
long restart_cases(unsigned long long *reached)
{
    const uint64_t none = 0xFFFFFull;
    std::vector<uint64_t> T(15 + 8, none);
    auto tr = [](uint64_t c, bool fin, uint64_t next, uint64_t ow) { return c | (fin ? SG_FINAL : 0ull) | (next << SG_NEXT_SHIFT) | (ow << SG_OW_SHIFT); };
    T[0] = tr(0, false, 3, 0); T[1] = tr(1, true, 6, 1); T[2] = tr(2, true, 9, 2); T[3 + 1] = tr(1, true, 12, 0);      // keys: "01" 0, "1" 1, "2" 2
    union { float f; uint32_t u; } neg, pos; neg.f = -3.0e38f; pos.f = 3.0e38f;
    const SegInfo info[3] = {{10, neg.u}, {11, pos.u}, {12, neg.u}};
    const uint32_t score[3] = {neg.u, pos.u, neg.u};
    const int32_t idcol[3] = {10, 11, 12};
    SegTables S; S.T = T.data(); S.info = info; S.initial = 0; S.cls_delim = 0xFFFDu; S.kind = SG_KIND_UNIGRAM; S.id_offset = 1; S.score = score;
    const std::vector<std::vector<uint16_t>> texts = {{2, 2, 0, 1}, {2, 2, 0, 1, 2, 2, 1}, {0, 1}, {1, 2, 0, 1, 0, 1, 2}, {2, 0, 0, 1, 2, SG_CLS_NONE, 2}};
    struct Out { std::vector<int32_t> id; std::vector<int> from, to; void put(int k, int v) { id.resize((size_t)k + 1 > id.size() ? (size_t)k + 1 : id.size()); id[(size_t)k] = v; }
                 void span(int k, int f, int t) { from.resize(id.size()); to.resize(id.size()); from[(size_t)k] = f; to[(size_t)k] = t; } void finish(int) {} };
    long diffs = 0;
    for (size_t t = 0; t < texts.size(); ++t) for (int mx : {100, 2}) {
        std::vector<uint16_t> cls = texts[t]; const int L = (int)cls.size(); cls.push_back(0);
        const uint16_t *cp = cls.data();
        auto cls_at = [cp](int i) -> uint32_t { return cp[i]; };
        std::vector<SegBest> best((size_t)L + 1);
        Out w;
        const int nw = seg_unigram_doc(S, cls_at, L, best.data(), w, mx, 7);
        for (int k = 0; k < 4; ++k) {
            Driver dr = DRIVERS[k]; dr.W = 16;
            std::vector<int32_t> ids; std::vector<int> from, to;
            const int ng = cut_doc(S, idcol, cp, L, 2, dr, (int)((t + (size_t)k) & 3), mx, 7, ids, from, to, reached);
            bool same = ng == nw;
            for (int i = 0; same && i < ng; ++i) same = ids[(size_t)i] == w.id[(size_t)i] && from[(size_t)i] == w.from[(size_t)i] && to[(size_t)i] == w.to[(size_t)i];
            if (!same) { ++diffs; fprintf(stderr, "unioffs: restart text %ld max_ids %d driver %d: %d tokens, the sequential form %d, or other values\n", (long)t, mx, k, ng, nw); }
        }
    }
    return diffs;
}

} // namespace

extern "C" {
// model_path == nullptr: the restart dictionary alone.  reached[3] += {restarts, spills, short ways out}.  -1: the model does not load or is not Unigram
long bft_unioffs_run(const char *model_path, unsigned long long *reached)
{
    if (!model_path) return restart_cases(reached);
    FILE *f = fopen(model_path, "rb");
    if (!f) return -1;
    std::vector<uint8_t> img; uint8_t buf[65536]; size_t k;
    while ((k = fread(buf, 1, sizeof buf, f)) > 0) img.insert(img.end(), buf, buf + k);
    fclose(f);
    Handle h; h.path = model_path;
    if (!build_model(h.m, img.data(), img.size()) || h.m.kind != KIND_UNIGRAM) return -1;
    bfo_model *o = bfo_set_model(img.data(), img.size());
    if (!o) return -1;
    const long r = model_cases(h, o, reached);
    bfo_free_model(o);
    return r;
}
}

#ifdef BF_UNIOFFS_MAIN
int main(int argc, char **argv)
{
    unsigned long long reached[3] = {0, 0, 0};
    long bad = bft_unioffs_run(nullptr, reached);
    for (int a = 1; a < argc; ++a) { const long r = bft_unioffs_run(argv[a], reached); bad += r < 0 ? 1 : r; }
    printf("unioffs: %ld differences; restarts %llu spills %llu short ways out %llu\n", bad, reached[0], reached[1], reached[2]);
    return bad == 0 && reached[0] && reached[1] && reached[2] ? 0 : 1;
}
#endif
