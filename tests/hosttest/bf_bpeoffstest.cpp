// bf_bpeoffstest.cpp -- TEST-ONLY: the offsets call of a BPE model on the wave program, on the host.  The SPANS instance of BpeWave
// (bf_bpe_wave_body.h: an id sits in the cell under its piece's first element) runs in the 64-fibre wave simulator on one batch, the documents
// it hands back go through BpeSeg with spans (bf_bpe_seg_body.h) as on the device, then every document takes what k_bpe_home_spans does per
// block of 64 cells (bf_bpe_home.h: the next id cell, from / to, the byte offsets).  Count, ids, first byte and last byte of every document are
// compared with the oracle's bfo_text_to_ids_with_offsets, for max_ids above the token counts, 3 and 1.
// bft_bpeoffs_run returns the number of differences; reached[4] += {documents handed back, tokens whose end came from the look-ahead mask,
// words of solve_big, words of unit_huge}.  With -DBF_BPEOFFS_MAIN the unit is a stand-alone program (bf_bpeoffs MODEL...), built under the
// address and undefined-behaviour sanitizers by blingfire_amd/build.py build_bpeoffs_san(); it is never loaded into python in that form.
//
// wave_emu.h defines its fibre switch as a global symbol and bf_wavetest.cpp of the same library includes it too: this unit's copy is weak
// (the assembler lets .weak override the header's .globl), so the library links one of the two identical routines.
__asm__(".weak wvemu_switch");
#include "wave_emu.h"
#include "../../blingfire_amd/csrc/bf_bpe_wave_body.h"
#include "../../blingfire_amd/csrc/bf_bpe_seg_body.h"
#include "../../blingfire_amd/csrc/bf_bpe_home.h"
#include "../../oracle/bf_oracle.h"
#include "hosttest.h"
#include "ws_sizes.h"

#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

using namespace bfa;
static_assert(BW_WORD_MAX <= BH_PIECE_MAX, "one block of look-ahead");

namespace {

// The wave programs are templates and the simulator's wv:: functions are static to the unit that includes wave_emu.h: an instance that
// bf_wavetest.cpp has too (BpeSeg<BsLds>) would be merged with that unit's at link time and run on the wrong unit's fibres.  LDS types of this
// unit's own give every instance here internal linkage.
struct OffsWaveLds : BwLds<1024, 256, 8> {};
struct OffsSegLds : BsLds {};

template <class Body> void in_waves(int nwaves, Body make)
{
    std::vector<const void *> wave_ids;
    wvemu::run_waves(nwaves, [&]() {
        const void *wid = (const void *)wvemu::g_cur->wave;
        size_t k = 0;
        for (; k < wave_ids.size(); ++k) if (wave_ids[k] == wid) break;
        if (k == wave_ids.size()) wave_ids.push_back(wid);
        make((int)k);
    });
}

std::string rep(const std::string &s, int n) { std::string r; for (int k = 0; k < n; ++k) r += s; return r; }

// the case table (tests/test_gpu_bpe_offsets.py runs the like on the device)
std::vector<std::string> case_docs()
{
    std::vector<std::string> d = {
        "", " ", "   ", "the", "unaffable", "hello world", " internationalization of pneumonoultramicroscopic words",
        "--------", "------------------------", rep("=", 48), rep("a", 40),                    // runs of one letter: more and more arcs (solve_big, unit_huge)
        rep("qxzjvk", 10) + "q", rep("qxzjvk", 10) + "qx", "in " + rep("a", 62) + " out",      // words of 62 and 63 elements: the second is handed back
        "caf\xC3\xA9 \xE6\x97\xA5\xE6\x9C\xAC \xF0\x9F\x98\x80\xF0\x9F\x98\x80 \xC2\xAA",       // 2-, 3- and 4-byte characters
        "ends with a piece of one letter x",
    };
    // documents of about 63 .. 193 elements of two-element words, behind a first word of three (a piece starts in the last cell of a block -- 63, 127 --
    // and the next one in the next block) and without it; and of 61-element words, whose ends come from the look-ahead mask
    for (int n : {63, 64, 65, 127, 128, 129, 193}) { d.push_back("bc" + rep(" a", (n - 3) / 2)); d.push_back(rep("a ", n / 2)); }
    d.push_back(rep(rep("qxzjvk", 10) + " ", 4));
    return d;
}

struct Out { std::vector<int32_t> id; std::vector<int> first, last; };

long model_cases(Handle &h, bfo_model *o, unsigned long long *reached)
{
    Model &m = h.m;
    const std::vector<std::string> docs = case_docs();
    const long ndocs = (long)docs.size();
    const int mul = m.dict_has_charmap ? 2 : 1, unk = 0;
    std::vector<int64_t> doc_off((size_t)ndocs + 1, 0);
    std::string text;
    for (long d = 0; d < ndocs; ++d) { text += docs[(size_t)d]; doc_off[(size_t)d + 1] = (int64_t)text.size(); }
    const size_t cells = (size_t)ws_sp_cells(mul, ndocs, (int64_t)text.size()), nd = (size_t)ws_doc_cells(ndocs);
    std::vector<uint16_t> stream(cells + (size_t)ws_sp_stream_slack, (uint16_t)0xEEEE);
    std::vector<int32_t> src_off(cells, -77), lens(nd, 0);
    for (long d = 0; d < ndocs; ++d) {
        std::vector<uint16_t> st; std::vector<int> so;
        if (!bft_sp_stream(m, docs[(size_t)d].data(), (int)docs[(size_t)d].size(), st, &so)) continue;
        const size_t slot = (size_t)mul * (size_t)(doc_off[(size_t)d] + d);
        lens[(size_t)d] = (int32_t)st.size();
        for (size_t k = 0; k < st.size(); ++k) { stream[slot + k] = st[k]; src_off[slot + k] = so[k]; }
    }
    long diffs = 0;
    for (int mx : {4096, 3, 1}) {
        std::vector<int32_t> tmp((size_t)ws_sp_tmp_cells(mul, ndocs, (int64_t)text.size()), -77), span(2 * cells, -77), counts(nd, -55), flags(nd, -55), list(nd, -1);
        std::vector<uint32_t> scratch((size_t)ws_bpe_scratch_words((int64_t)cells), 0xABABABABu);
        unsigned long long next_doc = 0, stats[16] = {0}; int status = 0;
        BpeWaveParams p;
        p.T = m.dict.t64.data(); p.info = (const SegInfo *)m.seg_info.data(); p.initial = m.dict.initial_base; p.cls_delim = m.sp_delim_code; p.id_offset = m.id_offset;
        p.prio = m.kind == KIND_BPE_MERGES ? m.bpe_prio.data() : nullptr; p.place_id = m.kind == KIND_BPE_MERGES ? m.bpe_place_id.data() : nullptr;
        p.stream = stream.data(); p.lens = lens.data(); p.doc_off = doc_off.data(); p.slot_mul = mul; p.ndocs = ndocs;
        p.ids_tmp = tmp.data(); p.counts = counts.data(); p.flags = flags.data(); p.max_ids = mx; p.next_doc = &next_doc; p.status = &status; p.stats = stats; p.scratch = scratch.data();
        if (!m.bpe_tab.empty()) { p.W = m.bpe_tab.data(); p.wbits = m.bpe_tab_bits; p.m0 = m.bpe_tab_m0; p.m1 = m.bpe_tab_m1; p.m2 = m.bpe_tab_m2; }
        typedef OffsWaveLds LDS;
        const int nwaves = 2;
        std::vector<LDS> lds((size_t)nwaves);
        memset((void *)lds.data(), 0xA5, sizeof(LDS) * (size_t)nwaves);
        in_waves(nwaves, [&](int k) { BpeWave<LDS, 4, 32, true, true> w(p, lds[(size_t)k]); w.run(3, k, nwaves); });
        // the documents handed back: k_bpe_flag_list, k_bpe_seg with spans
        unsigned int list_n = 0;
        for (long d = 0; d < ndocs; ++d) if (flags[(size_t)d] == 1) list[list_n++] = (int32_t)d;
        unsigned long long pool_used = 0, pool_need = 0;
        std::vector<uint8_t> pool((size_t)1 << 20);
        BpeSegParams q;
        q.T = p.T; q.info = p.info; q.initial = p.initial; q.cls_delim = p.cls_delim; q.id_offset = p.id_offset; q.kind = m.kind; q.prio = p.prio; q.place_id = p.place_id;
        q.unk_prio = bpe_unk_prio(m, unk); q.prio_bits = m.bpe_prio_bits;
        q.stream = p.stream; q.lens = p.lens; q.doc_off = p.doc_off; q.slot_mul = mul; q.list = list.data(); q.list_n = &list_n; q.narcs = nullptr; q.narcs_want = 0; q.ndocs = ndocs;
        q.ids_tmp = tmp.data(); q.span_tmp = span.data(); q.counts = counts.data(); q.max_ids = mx; q.unk = unk;
        next_doc = 0; q.next_doc = &next_doc; q.status = &status;
        q.pool = pool.data(); q.pool_bytes = pool.size(); q.pool_used = &pool_used; q.pool_need = &pool_need; q.stats = nullptr;
        OffsSegLds slds;
        if (list_n) in_waves(1, [&](int) { BpeSeg<OffsSegLds> w(q, slds); w.run(); });
        if (status) { fprintf(stderr, "bpeoffs: %s max_ids %d: status %d\n", h.path.c_str(), mx, status); return diffs + 1; }
        reached[0] += list_n; reached[2] += stats[9] + stats[10] + stats[11]; reached[3] += stats[7];
        for (long d = 0; d < ndocs; ++d) {
            const std::string &doc = docs[(size_t)d];
            const int n = (int)doc.size(), L = lens[(size_t)d], c = counts[(size_t)d];
            std::vector<char> s((size_t)n + 2, 'A');          // the oracle reads the byte in front of the string for a token made of the dummy prefix alone
            if (n) memcpy(s.data() + 1, doc.data(), (size_t)n);
            std::vector<int32_t> wi((size_t)mx); std::vector<int> ws((size_t)mx), we((size_t)mx);
            int want = bfo_text_to_ids_with_offsets(o, s.data() + 1, n, wi.data(), ws.data(), we.data(), mx, unk);
            want = want < 0 ? 0 : want > mx ? mx : want;
            const size_t slot = (size_t)mul * (size_t)(doc_off[(size_t)d] + d);
            const int32_t *cell = tmp.data() + slot, *so = src_off.data() + slot;
            const uint8_t *t = (const uint8_t *)doc.data();
            Out g;
            auto put = [&](int32_t id, int from, int to) { int a, b; bh_bytes(so, t, from, to, a, b); g.id.push_back(id); g.first.push_back(a); g.last.push_back(b); };
            if (flags[(size_t)d] == 1) for (int i = 0; i < c; ++i) put(cell[i], span[2 * (slot + (size_t)i)], span[2 * (slot + (size_t)i) + 1]);
            else for (int base = 0; base < L && (int)g.id.size() < c; base += BH_BLOCK) {      // k_bpe_home_spans, block by block
                unsigned long long own = 0, ahead = 0;
                for (int l = 0; l < BH_BLOCK; ++l) { if (base + l < L && cell[base + l] != BW_HOME_NONE) own |= 1ull << l; if (base + BH_BLOCK + l < L && cell[base + BH_BLOCK + l] != BW_HOME_NONE) ahead |= 1ull << l; }
                for (int l = 0; l < BH_BLOCK && (int)g.id.size() < c; ++l) if ((own >> l) & 1ull) {
                    int from, to;
                    bh_span(own, ahead, base, l, L, from, to);
                    if (bh_next_cell(own, ahead, l) >= BH_BLOCK) ++reached[1];
                    put(cell[base + l], from, to);
                }
            }
            bool same = c == want && (int)g.id.size() == want && flags[(size_t)d] >= 0;
            for (int i = 0; same && i < want; ++i) same = g.id[(size_t)i] == wi[(size_t)i] && g.first[(size_t)i] == ws[(size_t)i] && g.last[(size_t)i] == we[(size_t)i];
            if (!same) { ++diffs; fprintf(stderr, "bpeoffs: %s document %ld max_ids %d (handed back %d): %d tokens, the oracle %d, or other values\n", h.path.c_str(), d, mx, flags[(size_t)d], c, want); }
        }
    }
    return diffs;
}

} // namespace

extern "C" {
// -1: the model does not load or the BPE wave program does not admit it
long bft_bpeoffs_run(const char *model_path, unsigned long long *reached)
{
    FILE *f = fopen(model_path, "rb");
    if (!f) return -1;
    std::vector<uint8_t> img; uint8_t buf[65536]; size_t k;
    while ((k = fread(buf, 1, sizeof buf, f)) > 0) img.insert(img.end(), buf, buf + k);
    fclose(f);
    Handle h; h.path = model_path;
    if (!build_model(h.m, img.data(), img.size()) || !h.m.bpe_wave_ok || !h.m.bpe_seg_ok) return -1;
    bfo_model *o = bfo_set_model(img.data(), img.size());
    if (!o) return -1;
    const long r = model_cases(h, o, reached);
    bfo_free_model(o);
    return r;
}
}

#ifdef BF_BPEOFFS_MAIN
int main(int argc, char **argv)
{
    unsigned long long reached[4] = {0, 0, 0, 0};
    long bad = 0;
    for (int a = 1; a < argc; ++a) { const long r = bft_bpeoffs_run(argv[a], reached); bad += r < 0 ? 1 : r; }
    printf("bpeoffs: %ld differences; handed back %llu look-ahead ends %llu solve_big %llu unit_huge %llu\n", bad, reached[0], reached[1], reached[2], reached[3]);
    return bad == 0 && argc > 1 && reached[0] && reached[1] ? 0 : 1;
}
#endif
