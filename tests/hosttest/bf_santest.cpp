// bf_santest.cpp -- TEST-ONLY: the tokenizer lane programs and the model loader as a stand-alone program under the address and undefined-behaviour
// sanitizers (tests/test_sanitized_host.py builds it with -DBF_SANTEST_MAIN and links every unit of tests/hosttest, bf_model.cpp and the oracle
// into it; without the macro this unit is empty, so libbf_hosttest.so does not change).  Never loaded into python.
//
//   bf_santest ids    MODEL CASE    every TextToIds program the model is eligible for, each answer against the oracle linked in here
//   bf_santest flat   MODEL CASE    the flat program alone (ids and offsets, 7 ranges, max_ids 128): batches with documents at its size limit
//   bf_santest words  MODEL CASE    the words / sentences lexers, short and long form
//   bf_santest dict   MODEL CASE    the dictionary lookup (a document = a key of int32 symbols)
//   bf_santest w2h    MODEL CASE    the hyphenation lane program against the answers the case file carries
//   bf_santest loader PRISTINE CASE WORDS [LIST]   build_model on the pristine image and then on every image LIST names, the programs on every model
//                                                  that loads (WORDS: the hyphenator's catalogue; no answers compared: the oracle is not made for damaged images)
//
// Every input is copied into a heap block of exactly its size (n bytes of text, ndocs + 1 offsets), every output has exactly its capacity, and the
// emulators size their workspaces as the product does (ws_sizes.h): an access one element outside any of them is a sanitizer report.  The first
// difference from the oracle ends the program with a non-zero status.
//
// Case file: int64 {magic, ndocs, nbytes, unk, u_hy, nexpect, 0, 0}, int64 offsets[ndocs + 1], text[nbytes]; w2h: int64 expect_off[ndocs + 1],
// expect[nexpect] behind it.
#ifdef BF_SANTEST_MAIN
#include "hosttest.h"
#include "../../blingfire_amd/csrc/bf_batch.h"
#include "../../oracle/bf_oracle.h"

#include <sys/resource.h>
#include <sys/wait.h>
#include <unistd.h>
#include <chrono>
#include <csignal>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

using namespace bfa;

extern "C" {
int bft_emu_text_to_ids(void *hv, const char *s, int n, int32_t *ids, int max_ids, int unk);
int bft_emu_text_to_ids_with_offsets(void *hv, const char *s, int n, int32_t *ids, int32_t *starts, int32_t *ends, int max_ids, int unk);
int bft_emu_text_to_words(void *hv, const char *s, int n, char *out, int32_t *starts, int32_t *ends, int max_out);
int bft_emu_lex_tokens(void *hv, const char *s, int n, int mode, int long_form, int cap, int32_t *tags, int32_t *spans, int max_out, int *visited);
int bft_emu_dict_get_info(void *hv, const int32_t *key, int n, int32_t *info_id, int32_t *vals, int max_vals);
void bft_set_uni_cut(int w, int period);
void bft_set_uni_cut_k(int k);
void bft_set_uni_cut_quick(int v);
void bft_set_uni_seq(int v);
long bft_emu_wave_batch(void *hv, const uint8_t *text, long text_bytes, const int64_t *doc_off, long ndocs, int max_ids, int unk, int nwaves, int grab, int cfg,
                        int32_t *ids_out, long ids_cap, int64_t *id_off, unsigned long long *stats);
long bft_emu_wave_batch_offsets(void *hv, const uint8_t *text, long text_bytes, const int64_t *doc_off, long ndocs, int max_ids, int unk, int nwaves, int grab, int cfg,
                                int32_t *ids_out, int32_t *starts_out, int32_t *ends_out, long ids_cap, int64_t *id_off);
long bft_emu_bpe_wave_batch(void *hv, const uint8_t *text, long text_bytes, const int64_t *doc_off, long ndocs, int max_ids, int unk, int nwaves, int grab, int cfg,
                            int32_t *ids_out, long ids_cap, int64_t *id_off, int32_t *flags_out, unsigned long long *stats);
long bft_emu_bpe_seg_batch(void *hv, const uint8_t *text, const int64_t *doc_off, long ndocs, int max_ids, int unk, int nwaves, long pool_bytes,
                           int32_t *ids_out, long ids_cap, int64_t *id_off, int32_t *spans_out, int *status_out, unsigned long long *pool_used_out, unsigned long long *stats);
long bft_emu_flat_batch(void *hv, const uint8_t *text, long text_bytes, const int64_t *doc_off, long ndocs, int max_ids, int unk, int nwaves, int nranges,
                        int32_t *ids_out, long ids_cap, int64_t *id_off, unsigned long long *stats, long wrec_cap_in);
long bft_emu_flat_batch_offsets(void *hv, const uint8_t *text, long text_bytes, const int64_t *doc_off, long ndocs, int max_ids, int unk, int nwaves, int nranges,
                                int32_t *ids_out, int32_t *starts_out, int32_t *ends_out, long ids_cap, int64_t *id_off, unsigned long long *stats);
long long bft_w2h_batch(void *hv, const unsigned char *text, const long long *off, long long n, int u_hy, unsigned char *out, long long cap, long long *out_off);
}

namespace {

const int64_t CASE_MAGIC = 0x3153434e41534642ll;      // "BFSANCS1"
const int MAX_IDS[4] = {0, 1, 7, 128};

// a heap block of exactly n elements (one byte where n is 0: a pointer that may not be read at all)
template <class T> struct Exact {
    T *p; size_t n;
    explicit Exact(size_t count, int fill = 0) : p((T *)malloc(count ? count * sizeof(T) : 1)), n(count) { if (!p) { fprintf(stderr, "santest: out of memory\n"); exit(2); } if (count) memset((void *)p, fill, count * sizeof(T)); }
    Exact(const T *src, size_t count) : Exact(count) { if (count) memcpy((void *)p, src, count * sizeof(T)); }
    ~Exact() { free(p); }
    Exact(const Exact &) = delete;
    Exact &operator=(const Exact &) = delete;
};

struct Case {
    int64_t ndocs = 0, nbytes = 0, unk = 0, u_hy = 0, nexpect = 0;
    std::vector<int64_t> off, expect_off;
    std::vector<uint8_t> text, expect;
};

[[noreturn]] void die(const char *fmt, const char *a = "", long b = 0, long c = 0)
{
    fprintf(stderr, "santest: ");
    fprintf(stderr, fmt, a, b, c);
    fprintf(stderr, "\n");
    exit(1);
}

bool read_file(const char *path, std::vector<uint8_t> &out)
{
    FILE *f = fopen(path, "rb");
    if (!f) return false;
    out.clear();
    uint8_t buf[65536]; size_t k;
    while ((k = fread(buf, 1, sizeof buf, f)) > 0) out.insert(out.end(), buf, buf + k);
    fclose(f);
    return true;
}

Case read_case(const char *path)
{
    std::vector<uint8_t> raw;
    if (!read_file(path, raw) || raw.size() < 64) die("cannot read the case file %s", path);
    int64_t head[8];
    memcpy(head, raw.data(), sizeof head);
    Case c;
    if (head[0] != CASE_MAGIC || head[1] < 0 || head[2] < 0 || head[5] < 0) die("%s is not a case file", path);
    c.ndocs = head[1]; c.nbytes = head[2]; c.unk = head[3]; c.u_hy = head[4]; c.nexpect = head[5];
    size_t at = 64, need = at + (size_t)(c.ndocs + 1) * 8 + (size_t)c.nbytes + (c.nexpect ? (size_t)(c.ndocs + 1) * 8 + (size_t)c.nexpect : 0);
    if (raw.size() != need) die("%s: size %ld, expected %ld", path, (long)raw.size(), (long)need);
    c.off.resize((size_t)c.ndocs + 1); memcpy(c.off.data(), raw.data() + at, c.off.size() * 8); at += c.off.size() * 8;
    c.text.assign(raw.begin() + (long)at, raw.begin() + (long)at + c.nbytes); at += (size_t)c.nbytes;
    if (c.nexpect) {
        c.expect_off.resize((size_t)c.ndocs + 1); memcpy(c.expect_off.data(), raw.data() + at, c.expect_off.size() * 8); at += c.expect_off.size() * 8;
        c.expect.assign(raw.begin() + (long)at, raw.end());
    }
    for (int64_t d = 0; d < c.ndocs; ++d) if (c.off[(size_t)d] < 0 || c.off[(size_t)d + 1] < c.off[(size_t)d] || c.off[(size_t)d + 1] > c.nbytes) die("%s: offsets of document %ld", path, (long)d);
    return c;
}

// the handle of the emulators on an exactly sized heap copy of an image
bool load_image(Handle &h, const std::vector<uint8_t> &img)
{
    Exact<uint8_t> copy(img.data(), img.size());
    return build_model(h.m, copy.p, copy.n);
}

// ---- the oracle's answers for a batch: per document, once per max_ids
struct Want { std::vector<int32_t> ids, starts, ends; std::vector<int64_t> off; };

Want oracle_batch(const bfo_model *o, const Case &c, int max_ids, bool offsets)
{
    Want w; w.off.assign(1, 0);
    std::vector<int32_t> ids((size_t)(max_ids > 0 ? max_ids : 1)); std::vector<int> st(ids.size()), en(ids.size());
    for (int64_t d = 0; d < c.ndocs; ++d) {
        const int n = (int)(c.off[(size_t)d + 1] - c.off[(size_t)d]);
        // the oracle reads the byte in front of the string for a token made of the dummy prefix alone (as the reference does, tokdll:1527): its copy has one
        std::vector<char> s((size_t)n + 2, 'A');
        if (n) memcpy(s.data() + 1, c.text.data() + c.off[(size_t)d], (size_t)n);
        s[(size_t)n + 1] = 0;
        int k = offsets ? bfo_text_to_ids_with_offsets(o, s.data() + 1, n, ids.data(), st.data(), en.data(), max_ids, (int)c.unk) : bfo_text_to_ids(o, s.data() + 1, n, ids.data(), max_ids, (int)c.unk);
        if (k < 0) k = 0;
        if (k > max_ids) k = max_ids;
        for (int i = 0; i < k; ++i) { w.ids.push_back(ids[(size_t)i]); if (offsets) { w.starts.push_back(st[(size_t)i]); w.ends.push_back(en[(size_t)i]); } }
        w.off.push_back((int64_t)w.ids.size());
    }
    return w;
}

void same_batch(const char *what, int max_ids, int cfg, const Want &w, long r, const int32_t *ids, const int64_t *id_off, int64_t ndocs, const int32_t *starts = nullptr, const int32_t *ends = nullptr)
{
    if (r != (long)w.ids.size()) { fprintf(stderr, "santest: %s (max_ids %d, cfg %d): returned %ld, the oracle has %ld ids\n", what, max_ids, cfg, r, (long)w.ids.size()); exit(1); }
    for (int64_t d = 0; d <= ndocs; ++d) if (id_off[d] != w.off[(size_t)d]) { fprintf(stderr, "santest: %s (max_ids %d, cfg %d): id offset of document %ld is %ld, the oracle's %ld\n", what, max_ids, cfg, (long)d, (long)id_off[d], (long)w.off[(size_t)d]); exit(1); }
    for (size_t i = 0; i < w.ids.size(); ++i) {
        if (ids[i] != w.ids[i] || (starts && (starts[i] != w.starts[i] || ends[i] != w.ends[i]))) {
            fprintf(stderr, "santest: %s (max_ids %d, cfg %d): id %ld differs from the oracle's\n", what, max_ids, cfg, (long)i); exit(1);
        }
    }
}

// The per-document lane emulation: ids, and ids with offsets, every document in a block of its own.  compare = false: run only (damaged images).
void run_lanes(Handle &h, const bfo_model *o, const Case &c, const char *what, bool with_offsets, bool compare)
{
    for (int mi = 0; mi < 4; ++mi) {
        const int mx = MAX_IDS[mi];
        Want w, wo;
        if (compare) { w = oracle_batch(o, c, mx, false); if (with_offsets) wo = oracle_batch(o, c, mx, true); }
        for (int64_t d = 0; d < c.ndocs; ++d) {
            const int n = (int)(c.off[(size_t)d + 1] - c.off[(size_t)d]);
            Exact<char> s((const char *)c.text.data() + c.off[(size_t)d], (size_t)n);
            Exact<int32_t> ids((size_t)mx, 0x5a);
            const int k = bft_emu_text_to_ids(&h, s.p, n, ids.p, mx, (int)c.unk);
            if (compare) {
                const int64_t a = w.off[(size_t)d], z = w.off[(size_t)d + 1];
                if (k != (int)(z - a) || (k > 0 && memcmp(ids.p, w.ids.data() + a, (size_t)k * 4) != 0)) { fprintf(stderr, "santest: %s, document %ld, max_ids %d: %d ids, the oracle %ld, or other ids\n", what, (long)d, mx, k, (long)(z - a)); exit(1); }
            } else if (k > mx) die("%s: more ids than max_ids", what);
            if (!with_offsets) continue;
            Exact<int32_t> ids2((size_t)mx, 0x5a), st((size_t)mx, 0x5a), en((size_t)mx, 0x5a);
            const int k2 = bft_emu_text_to_ids_with_offsets(&h, s.p, n, ids2.p, st.p, en.p, mx, (int)c.unk);
            if (compare) {
                const int64_t a = wo.off[(size_t)d], z = wo.off[(size_t)d + 1];
                bool ok = k2 == (int)(z - a);
                for (int i = 0; ok && i < k2; ++i) ok = ids2.p[i] == wo.ids[(size_t)(a + i)] && st.p[i] == wo.starts[(size_t)(a + i)] && en.p[i] == wo.ends[(size_t)(a + i)];
                if (!ok) { fprintf(stderr, "santest: %s with offsets, document %ld, max_ids %d differs from the oracle\n", what, (long)d, mx); exit(1); }
            }
        }
    }
}

// Every batch program the model is eligible for.  The batch's text and offsets are exact heap blocks; ids_cap is the total the oracle has (compare) or
// what max_ids allows (damaged images).
void run_batches(Handle &h, const bfo_model *o, const Case &c, bool compare, long pool_bytes, bool flat_only = false)
{
    const Model &m = h.m;
    Exact<uint8_t> text(c.text.data(), c.text.size());
    Exact<int64_t> off(c.off.data(), c.off.size());
    const long nd = (long)c.ndocs, nb = (long)c.nbytes; const int unk = (int)c.unk;
    Exact<unsigned long long> stats(16);      // the emulators' instances count (the tests read the counters; here they only need their 16 places)
    for (int mi = 0; mi < 4; ++mi) {
        const int mx = MAX_IDS[mi];
        if (flat_only && mx != 128) continue;
        Want w, wo;
        if (compare) { w = oracle_batch(o, c, mx, false); wo = oracle_batch(o, c, mx, true); }
        const size_t cap = compare ? w.ids.size() : (size_t)mx * (size_t)nd;
        const size_t capo = compare ? wo.ids.size() : cap;
        if (m.kind == KIND_WP && m.wave_ok && !flat_only) {
            static const int WV[6][2] = {{1, 8}, {3, 2}, {2, 8}, {1, 8}, {4, 2}, {2, 4}};      // waves, documents per grab of cfg 0 .. 5
            for (int cfg = 0; cfg < 6; ++cfg) {
                Exact<int32_t> ids(cap, 0x5a); Exact<int64_t> ido((size_t)nd + 1, 0x5a);
                const long r = bft_emu_wave_batch(&h, text.p, nb, off.p, nd, mx, unk, WV[cfg][0], WV[cfg][1], cfg, ids.p, (long)cap, ido.p, stats.p);
                if (compare) same_batch("wave program", mx, cfg, w, r, ids.p, ido.p, nd);
            }
            for (int cfg = 0; cfg < 2; ++cfg) {      // the offsets instance: shipped, and the smallest ring and queue
                Exact<int32_t> ids(capo, 0x5a), st(capo, 0x5a), en(capo, 0x5a); Exact<int64_t> ido((size_t)nd + 1, 0x5a);
                const long r = bft_emu_wave_batch_offsets(&h, text.p, nb, off.p, nd, mx, unk, cfg ? 3 : 2, cfg ? 2 : 8, cfg, ids.p, st.p, en.p, (long)capo, ido.p);
                if (compare) same_batch("wave program, offsets instance", mx, cfg, wo, r, ids.p, ido.p, nd, st.p, en.p);
                else if (r == -9 || r == -12) continue;      // (a damaged image: more ids than the room, spans the harness cannot map)
            }
        }
        if (m.kind == KIND_WP && m.wave_ok && m.flat_ok) {
            static const int NR[3] = {1, 7, 64};
            for (int k = flat_only ? 1 : 0; k < (flat_only ? 2 : 3); ++k) {
                Exact<int32_t> ids(cap, 0x5a); Exact<int64_t> ido((size_t)nd + 1, 0x5a);
                const long r = bft_emu_flat_batch(&h, text.p, nb, off.p, nd, mx, unk, 2, NR[k], ids.p, (long)cap, ido.p, stats.p, 0);
                if (compare) same_batch("flat program", mx, NR[k], w, r, ids.p, ido.p, nd);
                Exact<int32_t> ids2(capo, 0x5a), st(capo, 0x5a), en(capo, 0x5a); Exact<int64_t> ido2((size_t)nd + 1, 0x5a);
                const long r2 = bft_emu_flat_batch_offsets(&h, text.p, nb, off.p, nd, mx, unk, 2, NR[k], ids2.p, st.p, en.p, (long)capo, ido2.p, stats.p);
                if (compare) same_batch("flat program with offsets", mx, NR[k], wo, r2, ids2.p, ido2.p, nd, st.p, en.p);
            }
        }
        if (m.kind != KIND_WP && m.bpe_wave_ok) {
            for (int cfg = 0; cfg < 2; ++cfg) {
                Exact<int32_t> ids(cap, 0x5a), flags((size_t)nd + 1, 0x5a); Exact<int64_t> ido((size_t)nd + 1, 0x5a);
                const long r = bft_emu_bpe_wave_batch(&h, text.p, nb, off.p, nd, mx, unk, cfg ? 3 : 1, cfg ? 2 : 8, cfg, ids.p, (long)cap, ido.p, flags.p, stats.p);
                if (compare) same_batch("BPE wave program", mx, cfg, w, r, ids.p, ido.p, nd);
            }
        }
        if (m.kind != KIND_WP && m.bpe_seg_ok) {
            // once with a pool that holds every document, once with one small enough that some do not fit: those have no ids, the others the oracle's
            for (int small = 0; small < 2; ++small) {
                Exact<int32_t> ids(cap, 0x5a); Exact<int64_t> ido((size_t)nd + 1, 0x5a);
                int status = 0; unsigned long long used = 0;
                const long r = bft_emu_bpe_seg_batch(&h, text.p, off.p, nd, mx, unk, 2, small ? pool_bytes : (64l << 20), ids.p, (long)cap, ido.p, nullptr, &status, &used, stats.p);
                if (!compare) continue;
                if (!small) { if (status != 0) die("BPE seg program: status %s%ld with the large pool", "", status); same_batch("BPE seg program", mx, 0, w, r, ids.p, ido.p, nd); continue; }
                if (r < 0) die("BPE seg program, small pool: returned %s%ld", "", r);
                long dropped = 0;
                for (long d = 0; d < nd; ++d) {
                    const int64_t n = ido.p[d + 1] - ido.p[d], a = w.off[(size_t)d], z = w.off[(size_t)d + 1];
                    if (n == 0 && z > a) { ++dropped; continue; }
                    if (n != z - a || (n > 0 && memcmp(ids.p + ido.p[d], w.ids.data() + a, (size_t)n * 4) != 0)) die("BPE seg program, small pool: document %s%ld differs from the oracle", "", d);
                }
                if (dropped > 0 && !(status & BF_STATUS_POOL)) die("BPE seg program, small pool: %s%ld documents without ids, status %ld", "", dropped, status);
                if (mx == 128) printf("bpe_seg small pool: %ld of %ld documents did not fit\n", dropped, nd);
            }
        }
    }
}

// The dictionary entry with the largest key: from the initial state down to a leaf along the transition with the LARGEST output weight of every state
// (the classes of the path; empty when the walk does not end on the last key).  A document or a lookup key made of it reads the last row of every
// table the key indexes (info rows, scores, priorities, K2I): no fuzz document reaches it by chance, and a table one row short shows nowhere else.
std::vector<uint32_t> last_key_classes(const Model &m)
{
    std::vector<uint32_t> path;
    if (!m.has_seg || m.dict.t64.empty() || m.dict.nclasses <= 0 || m.i2info_id.empty()) return path;
    uint64_t base = m.dict.initial_base, key = 0;
    for (int depth = 0; depth < 4096; ++depth) {
        int best = -1; uint64_t best_ow = 0;
        for (int c = 0; c < m.dict.nclasses; ++c) {
            const uint64_t at = base + (uint64_t)c;
            if (at >= m.dict.t64.size() || (m.dict.t64[at] & T64_CLS_MASK) != (uint64_t)c) continue;
            const uint64_t ow = m.dict.t64[at] >> T64_OW_SHIFT;
            if (best < 0 || ow >= best_ow) { best = c; best_ow = ow; }
        }
        if (best < 0) break;
        path.push_back((uint32_t)best);
        key += best_ow;
        base = (m.dict.t64[base + (uint64_t)best] >> T64_NEXT_SHIFT) & T64_NEXT_MASK;
    }
    if (key + 1 != m.i2info_id.size()) path.clear();
    return path;
}

// the largest code point (or byte) `map` gives the class c, -1: none
int code_point_of(const TwoLevelMap &map, uint32_t c, bool bytes)
{
    for (int cp = bytes ? 255 : 0x10FFFF; cp >= 0; --cp) if ((cp < 0xD800 || cp > 0xDFFF) && map.get(cp) == c) return cp;
    return -1;
}

// the last key as a document (empty: a class of the path has no code point or byte of its own in the prologue's map)
std::vector<uint8_t> last_key_doc(const Model &m)
{
    std::vector<uint8_t> doc;
    for (uint32_t c : last_key_classes(m)) {
        const int cp = code_point_of(m.sp_cpmap, c, m.use_bytes);
        if (cp < 0) return std::vector<uint8_t>();
        if (m.use_bytes || cp < 0x80) doc.push_back((uint8_t)cp);
        else if (cp < 0x800) { doc.push_back((uint8_t)(0xC0 | (cp >> 6))); doc.push_back((uint8_t)(0x80 | (cp & 63))); }
        else if (cp < 0x10000) { doc.push_back((uint8_t)(0xE0 | (cp >> 12))); doc.push_back((uint8_t)(0x80 | ((cp >> 6) & 63))); doc.push_back((uint8_t)(0x80 | (cp & 63))); }
        else { doc.push_back((uint8_t)(0xF0 | (cp >> 18))); doc.push_back((uint8_t)(0x80 | ((cp >> 12) & 63))); doc.push_back((uint8_t)(0x80 | ((cp >> 6) & 63))); doc.push_back((uint8_t)(0x80 | (cp & 63))); }
    }
    return doc;
}

void run_ids(Handle &h, const bfo_model *o, const Case &c0, bool compare, long pool_bytes)
{
    const Model &m = h.m;
    Case c = c0;
    const std::vector<uint8_t> key_doc = compare && c.ndocs > 0 ? last_key_doc(m) : std::vector<uint8_t>();
    if (!key_doc.empty()) {
        // in front of the batch's last document, which stays the last bytes of the batch
        const int64_t at = c.off[(size_t)c.ndocs - 1];
        c.text.insert(c.text.begin() + at, key_doc.begin(), key_doc.end());
        c.off.insert(c.off.begin() + (c.ndocs - 1), at);
        for (size_t d = (size_t)c.ndocs; d < c.off.size(); ++d) c.off[d] += (int64_t)key_doc.size();
        c.ndocs += 1; c.nbytes += (int64_t)key_doc.size();
        printf("last key document: %ld bytes\n", (long)key_doc.size());
    }
    if (m.kind == KIND_WP) { if (m.has_wbd && !m.lexer_void) run_lanes(h, o, c, "lexer lane program", true, compare); }
    else if (m.kind == KIND_UNIGRAM) {
        run_lanes(h, o, c, "Unigram lane form", true, compare);
        static const int CUT[5][3] = {{32, 1, 3}, {32, 3, 3}, {64, 1 << 30, 1}, {32, 32, 3}, {32, 8, 4}};      // ring, emission period, transitions per trip (test_tables_and_emu.py)
        for (int k = 0; k < 5; ++k) {
            bft_set_uni_cut(CUT[k][0], CUT[k][1]); bft_set_uni_cut_k(CUT[k][2]); bft_set_uni_cut_quick(k == 1 ? 0 : 1);
            run_lanes(h, o, c, "Unigram cut form", false, compare);
        }
        bft_set_uni_cut(0, 1); bft_set_uni_cut_k(3); bft_set_uni_cut_quick(1);
        bft_set_uni_seq(1);
        run_lanes(h, o, c, "Unigram sequential restatement", true, compare);
        bft_set_uni_seq(0);
    } else if (m.kind == KIND_BPE || m.kind == KIND_BPE_OPT || m.kind == KIND_BPE_MERGES) run_lanes(h, o, c, "BPE lane program", true, compare);
    else return;
    run_batches(h, o, c, compare, pool_bytes);
}

// the words (mode 1) and sentences (mode 2) lexers: the sequential lane program against the long-document form, token for token, also with a triple
// buffer that fills in the middle; mode 1 against the oracle's TextToWords
void run_words(Handle &h, const bfo_model *o, const Case &c, bool compare)
{
    if (h.m.kind != KIND_WP || !h.m.has_wbd || h.m.lexer_void) return;
    long ntok = 0;
    for (int64_t d = 0; d < c.ndocs; ++d) {
        const int n = (int)(c.off[(size_t)d + 1] - c.off[(size_t)d]);
        if (n <= 0) continue;
        Exact<char> s((const char *)c.text.data() + c.off[(size_t)d], (size_t)n);
        for (int mode = 1; mode <= 2; ++mode) {
            const int caps[3] = {0, 3, n / 9 > 1 ? n / 9 : 1};
            for (int q = 0; q < 3; ++q) {
                Exact<int32_t> ta((size_t)n, 0x5a), sa(2 * (size_t)n, 0x5a), tb((size_t)n, 0x5a), sb(2 * (size_t)n, 0x5a);
                const int a = bft_emu_lex_tokens(&h, s.p, n, mode, 0, caps[q], ta.p, sa.p, n, nullptr);
                const int b = bft_emu_lex_tokens(&h, s.p, n, mode, 1, caps[q], tb.p, sb.p, n, nullptr);
                const int k = a < n ? a : n;      // (the count may exceed the room; what is written does not)
                if (compare && (a != b || (k > 0 && (memcmp(ta.p, tb.p, (size_t)k * 4) != 0 || memcmp(sa.p, sb.p, (size_t)k * 8) != 0)))) die("lexer, document %s%ld, mode %ld: the long form differs from the sequential program", "", (long)d, mode);
                if (a > 0) ntok += a;
            }
        }
        const int mo = 4 * n + 8;
        Exact<char> out((size_t)mo, 0x5a); Exact<int32_t> st((size_t)mo, 0x5a), en((size_t)mo, 0x5a);
        const int r = bft_emu_text_to_words(&h, s.p, n, out.p, st.p, en.p, mo);
        if (!compare) continue;
        std::vector<char> s2((size_t)n + 2, 'A'); memcpy(s2.data() + 1, s.p, (size_t)n); s2[(size_t)n + 1] = 0;
        std::vector<char> wout((size_t)mo + 4, 0x5a); std::vector<int> wst((size_t)mo, 0), wen((size_t)mo, 0);
        const int wr = bfo_text_to_words_with_offsets(o, s2.data() + 1, n, wout.data(), wst.data(), wen.data(), mo);
        if (r != wr || (r > 0 && memcmp(out.p, wout.data(), (size_t)r) != 0)) die("TextToWords, document %s%ld differs from the oracle", "", (long)d);
        int words = 0;
        for (int i = 0; i + 1 < r; ++i) if (out.p[i] == ' ') ++words;
        if (r > 1) ++words;
        for (int i = 0; i < words; ++i) if (st.p[i] != wst[(size_t)i] || en.p[i] != wen[(size_t)i]) die("TextToWords, document %s%ld: offsets differ from the oracle's", "", (long)d);
    }
    printf("words ok: %ld tokens\n", ntok);
}

void run_dict(Handle &h, const bfo_model *o, const Case &c, bool compare)
{
    if (!h.m.has_seg || h.m.k2i.empty()) { if (compare) die("the model has no dictionary to look up%s", ""); return; }
    long found = 0;
    // behind the case's keys: the last key of the dictionary, symbol by symbol (a left-to-right dictionary whose classes all have a symbol)
    std::vector<int32_t> last;
    if (compare && h.m.dict_direction == 0 && !h.m.dict_ignore_case) {
        for (uint32_t cl : last_key_classes(h.m)) { const int cp = code_point_of(h.m.dict_clsmap, cl, false); if (cp < 0) { last.clear(); break; } last.push_back(cp); }
    }
    for (int64_t d = 0; d < c.ndocs + (last.empty() ? 0 : 1); ++d) {
        const int n = d < c.ndocs ? (int)((c.off[(size_t)d + 1] - c.off[(size_t)d]) / 4) : (int)last.size();
        Exact<int32_t> key((size_t)n);
        if (n) memcpy(key.p, d < c.ndocs ? (const void *)(c.text.data() + c.off[(size_t)d]) : (const void *)last.data(), (size_t)n * 4);
        Exact<int32_t> vals(8, 0); int32_t id = 0;
        for (int i = 0; i < 8; ++i) vals.p[i] = -7;
        const int r = bft_emu_dict_get_info(&h, key.p, n, &id, vals.p, 8);
        if (!compare) continue;
        int want[8]; for (int i = 0; i < 8; ++i) want[i] = -7;
        const int wr = bfo_dict_get_info(o, key.p, n, want, 8), wi = bfo_dict_get_info_id(o, key.p, n);
        if (r != wr || id != wi || memcmp(vals.p, want, sizeof want) != 0) die("dictionary lookup, key %s%ld differs from the oracle", "", (long)d);
        found += wi != -1;
        if (d == c.ndocs) printf("last key: %d symbols, info id %d\n", n, wi);
    }
    printf("dict ok: %ld of %ld keys found\n", found, (long)c.ndocs);
}

// the hyphenation lane program: the batch into exactly the bytes the expected answers take, and into one byte less
void run_w2h(Handle &h, const Case &c, bool compare)
{
    if (!h.m.w2h_ready) { if (compare) die("the model has no usable [w2h]%s", ""); return; }
    Exact<unsigned char> text(c.text.data(), c.text.size());
    std::vector<long long> off64(c.off.begin(), c.off.end());
    Exact<long long> off(off64.data(), off64.size());
    const long long want_total = compare ? (long long)c.expect.size() : 8 * (long long)c.nbytes + 16;
    for (int less = 0; less < 2; ++less) {
        const long long cap = want_total - less < 0 ? 0 : want_total - less;
        Exact<unsigned char> out((size_t)cap, 0x5a); Exact<long long> out_off((size_t)c.ndocs + 1, 0x5a);
        const long long r = bft_w2h_batch(&h, text.p, off.p, c.ndocs, (int)c.u_hy, out.p, cap, out_off.p);
        if (!compare) continue;
        if (r != want_total) die("hyphenation: %s%ld bytes, expected %ld", "", (long)r, (long)want_total);
        for (int64_t d = 0; d <= c.ndocs; ++d) if (out_off.p[d] != c.expect_off[(size_t)d]) die("hyphenation: offset of word %s%ld", "", (long)d);
        if (cap && memcmp(out.p, c.expect.data(), (size_t)cap) != 0) die("hyphenation: the bytes differ%s", "");
    }
    printf("w2h ok: %ld words, %lld bytes\n", (long)c.ndocs, want_total);
}

// [i2w]: what IdsToText reads -- every token's bytes lie inside the data
void run_i2w(const Model &m)
{
    if (!m.has_i2w) return;
    if (m.i2w_off.empty()) die("a loaded [i2w] without offsets%s", "");
    unsigned long long sum = 0;
    for (size_t i = 0; i + 1 < m.i2w_off.size(); ++i) {
        if (m.i2w_off[i] > m.i2w_off[i + 1] || m.i2w_off[i + 1] > m.i2w_data.size()) die("a loaded [i2w]: token %s%ld lies outside the data", "", (long)i);
        for (uint32_t k = m.i2w_off[i]; k < m.i2w_off[i + 1]; ++k) sum += m.i2w_data[k];
    }
    (void)sum;
}

// the image being loaded and run; an image that does not finish within the limit ends the program at once, by name
const char *g_image = "";
void on_alarm(int)
{
    const char a[] = "santest: no end within the time limit: ";
    if (write(2, a, sizeof a - 1) < 0 || write(2, g_image, strlen(g_image)) < 0 || write(2, "\n", 1) < 0) _exit(3);
    _exit(3);
}

double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
long peak_rss_kb() { struct rusage u; getrusage(RUSAGE_SELF, &u); return u.ru_maxrss; }

// one image: build_model on an exact copy, then every program the model allows over the catalogue.  1 loaded, 0 refused
int load_and_run(const std::vector<uint8_t> &img, const Case &cat, const Case *words, const char *name)
{
    Handle h;
    const bool ok = load_image(h, img);
    if (!ok) {
        if (h.m.error.empty()) die("%s: build_model returned false without an error text", name);
        return 0;
    }
    if (!h.m.error.empty()) die("%s: build_model returned true with an error text", name);
    run_i2w(h.m);
    if (h.m.kind == KIND_W2H || h.m.w2h_ready) { if (words) run_w2h(h, *words, false); }
    if (h.m.kind != KIND_I2W && h.m.kind != KIND_W2H) {
        run_ids(h, nullptr, cat, false, 16 << 10);
        if (h.m.kind == KIND_WP) {
            if (h.m.has_wbd && !h.m.lexer_void) for (int64_t d = 0; d < cat.ndocs; ++d) {
                const int n = (int)(cat.off[(size_t)d + 1] - cat.off[(size_t)d]);
                if (n <= 0) continue;
                Exact<char> s((const char *)cat.text.data() + cat.off[(size_t)d], (size_t)n);
                const int caps[3] = {0, 3, n / 9 > 1 ? n / 9 : 1};
                for (int mode = 1; mode <= 2; ++mode) for (int q = 0; q < 3; ++q) for (int lf = 0; lf < 2; ++lf) {
                    Exact<int32_t> t((size_t)n, 0x5a), sp(2 * (size_t)n, 0x5a);
                    (void)bft_emu_lex_tokens(&h, s.p, n, mode, lf, caps[q], t.p, sp.p, n, nullptr);
                }
                const int mo = 4 * n + 8;
                Exact<char> out((size_t)mo, 0x5a); Exact<int32_t> st((size_t)mo, 0x5a), en((size_t)mo, 0x5a);
                (void)bft_emu_text_to_words(&h, s.p, n, out.p, st.p, en.p, mo);
            }
        } else if (h.m.has_seg && !h.m.k2i.empty()) {
            // keys for the dictionary: the catalogue's documents as symbols
            for (int64_t d = 0; d < cat.ndocs; ++d) {
                const int n = (int)(cat.off[(size_t)d + 1] - cat.off[(size_t)d]);
                Exact<int32_t> key((size_t)n);
                for (int i = 0; i < n; ++i) key.p[i] = cat.text[(size_t)cat.off[(size_t)d] + (size_t)i];
                Exact<int32_t> vals(8); int32_t id = 0;
                (void)bft_emu_dict_get_info(&h, key.p, n, &id, vals.p, 8);
            }
        }
    }
    return 1;
}

int main_loader(int argc, char **argv)
{
    if (argc < 5) die("usage: bf_santest loader PRISTINE CASE WORDS-CASE [LIST]%s", "");
    std::vector<uint8_t> img;
    if (!read_file(argv[2], img)) die("cannot read %s", argv[2]);
    const Case cat = read_case(argv[3]);
    const Case words = read_case(argv[4]); const Case *wp = &words;
    if (argc < 6) {
        // the baselines alone, in a child of this program: a process started by a large parent reports the parent's peak RSS as its own
        // (the peak is carried over when the program is replaced), a child forked here starts from this program's own
        fflush(stdout);
        const pid_t pid = fork();
        if (pid < 0) die("fork failed%s", "");
        if (pid == 0) {
            const double t0 = now_s();
            if (load_and_run(img, cat, wp, argv[2]) != 1) die("the pristine image %s does not load", argv[2]);
            printf("baseline seconds %.3f rss_kb %ld\n", now_s() - t0, peak_rss_kb());
            fflush(stdout);
            exit(0);
        }
        int st = 0;
        if (waitpid(pid, &st, 0) != pid) die("waitpid failed%s", "");
        return WIFEXITED(st) ? WEXITSTATUS(st) : 1;
    }
    const double t0 = now_s();
    if (load_and_run(img, cat, wp, argv[2]) != 1) die("the pristine image %s does not load", argv[2]);
    const double base = now_s() - t0, limit = 10.0 * base + 1.0;
    printf("baseline seconds %.3f\n", base);
    fflush(stdout);
    std::vector<uint8_t> list;
    if (!read_file(argv[5], list)) die("cannot read %s", argv[5]);
    long loaded = 0, refused = 0; double slowest = 0;
    signal(SIGALRM, on_alarm);
    size_t at = 0;
    while (at < list.size()) {
        size_t e = at; while (e < list.size() && list[e] != '\n') ++e;
        const std::string path((const char *)list.data() + at, e - at);
        at = e + 1;
        if (path.empty()) continue;
        if (!read_file(path.c_str(), img)) die("cannot read %s", path.c_str());
        printf("image %s\n", path.c_str()); fflush(stdout);      // (a sanitizer report names no image: the last line printed does)
        const double t1 = now_s();
        g_image = path.c_str();
        alarm((unsigned)limit + 2);      // (whole seconds: the exact limit is checked below, this ends what never returns)
        const int r = load_and_run(img, cat, wp, path.c_str());
        alarm(0);
        const double dt = now_s() - t1;
        if (dt > slowest) slowest = dt;
        if (dt > limit) { fprintf(stderr, "santest: %s took %.3f s, the limit is %.3f s (10 x the pristine image's %.3f s + 1 s)\n", path.c_str(), dt, limit, base); return 3; }
        if (r) ++loaded; else ++refused;
    }
    printf("loader ok: loaded %ld refused %ld slowest %.3f limit %.3f rss_kb %ld\n", loaded, refused, slowest, limit, peak_rss_kb());
    return 0;
}

} // namespace

int main(int argc, char **argv)
{
    if (argc < 2) die("usage: bf_santest ids|flat|words|dict|w2h|loader ...%s", "");
    const std::string mode = argv[1];
    if (mode == "loader") return main_loader(argc, argv);
    if (argc < 4) die("usage: bf_santest %s MODEL CASE", argv[1]);
    std::vector<uint8_t> img;
    if (!read_file(argv[2], img)) die("cannot read %s", argv[2]);
    const Case c = read_case(argv[3]);
    Handle h; h.path = argv[2];
    if (!load_image(h, img)) die("the model does not load: %s", h.m.error.c_str());
    if (mode == "w2h") { run_w2h(h, c, true); return 0; }
    bfo_model *o = bfo_set_model(img.data(), img.size());
    if (!o) die("the oracle does not load %s", argv[2]);
    if (mode == "ids") {
        run_ids(h, o, c, true, argc > 4 ? atol(argv[4]) : (16l << 10));
        printf("ids ok: kind %d wave %d flat %d bpe_wave %d bpe_seg %d, %ld documents, %ld bytes\n", h.m.kind, (int)h.m.wave_ok, (int)h.m.flat_ok, (int)h.m.bpe_wave_ok, (int)h.m.bpe_seg_ok, (long)c.ndocs, (long)c.nbytes);
    } else if (mode == "flat") {      // the flat program alone, once: batches with documents at its size limit
        if (!h.m.flat_ok) die("%s is not in flat form", argv[2]);
        run_batches(h, o, c, true, 0, true);
        printf("flat ok: %ld documents, %ld bytes\n", (long)c.ndocs, (long)c.nbytes);
    } else if (mode == "words") run_words(h, o, c, true);
    else if (mode == "dict") run_dict(h, o, c, true);
    else die("unknown mode %s", argv[1]);
    bfo_free_model(o);
    return 0;
}
#endif
