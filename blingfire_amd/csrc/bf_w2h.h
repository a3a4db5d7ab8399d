// bf_w2h.h -- the word hyphenator's lane programs.
//
// Reproduces, on the re-laid-out tables of bf_model.h (Model::w2h*), the reference
//   WordHyphenationWithModel                  (blingfiretools/blingfiretokdll/blingfiretokdll.cpp:818-911)
//   FAHyphInterpreter_core_t<int>::Process    (blingfirecompile.library/inc/FAHyphInterpreter_core_t.h:136-267)
//
// The reference starts a walk of the pattern automaton at every position `From` of the anchor-padded word and lays the pattern of every
// final state it passes over the output slots: don't-care is skipped, an unknown slot takes the value, a slot that holds another value
// becomes CONFLICT.  Nothing is carried from one `From` to the next, and -- with pattern values in 0 .. HYPH_DONT_CARE only, which the
// loader checks -- a slot's end value does not depend on the order of the overlays: it is the one value the slot saw, or CONFLICT if it
// saw two.  So every (word, From) is a lane of its own (w2h_walk) that ORs `1 << value` into one byte per slot, and a slot is resolved
// from its byte afterwards (w2h_hyphen_after).
//
// Four pieces, each written once as BF_HD code: the HIP kernels (bf_kernels_w2h.hip) run them per lane; tests/hosttest compiles the same
// header for the host and drives them sequentially against the reference (test-only: the product library never hyphenates on the CPU).
//
// Position stream: word w owns the elements [w2h_slot(word_off[w], w), + characters + 2) of a uint16 stream: the left anchor's class, the
// class of every character, the right anchor's class.  (A character takes at least one byte, so slots never overlap and need no scan.)
// Once the walks of a word are done its elements 1 .. characters are overwritten with the "a hyphen follows" flags the copy reads.
#pragma once
#include <stdint.h>
#include "bf_model.h"

#if !defined(BF_HD)
#if defined(__HIPCC__)
#define BF_HD __host__ __device__ __forceinline__
#else
#define BF_HD inline
#endif
#endif

namespace bfa {

constexpr int W2H_MAX_CHARS = 300;        // FALimits::MaxWordSize: what lies behind the 300th character is not looked at (tokdll:843-849)

struct W2hTables {
    const uint64_t *T;                    // T64 entries (bf_model.h); the output-weight field of a transition into a final state = offset of its pattern
    const uint8_t *pats;                  // [length low, length high, values ...]
    const uint16_t *cp_l1; const uint32_t *cp_pages;      // Model::w2h_cpmap
    uint32_t initial, cls_l, cls_r;
    int min_pat_len, no_hyph_len;
};

BF_HD int64_t w2h_slot(int64_t word_off_w, int64_t w) { return word_off_w + 2 * w; }

// Decodes the word s[0 .. n) as FAStrUtf8ToArray does (FAUtf8Utils.cpp:233-270 and 121-196: BOM skipped, strict UTF-8, at most 300 characters)
// and writes its slot of the position stream.  Returns the number of characters; 0 = the single call answers 0 or -1 (empty, too long for the
// reference's int, invalid UTF-8 within the first 300 characters, nothing but a BOM).  *src_bytes: bytes of those characters (BOM not counted).
BF_HD int w2h_prep_word(const W2hTables &t, const uint8_t *s, int64_t n, uint16_t *cls, int *src_bytes)
{
    *src_bytes = 0;
    if (n <= 0 || n > 1000000000) return 0;                                      // tokdll:832-837
    const int bom = (n >= 3 && s[0] == 0xEF && s[1] == 0xBB && s[2] == 0xBF) ? 3 : 0;
    int64_t pos = bom; int nch = 0;
    while (pos < n && nch < W2H_MAX_CHARS) {
        const uint32_t b0 = s[pos];
        int len = 1, cp = (int)b0;
        if (b0 >= 0x80) {
            if ((b0 & 0xE0) == 0xC0) { len = 2; cp = (int)(b0 & 0x1F); }
            else if ((b0 & 0xF0) == 0xE0) { len = 3; cp = (int)(b0 & 0x0F); }
            else if ((b0 & 0xF8) == 0xF0) { len = 4; cp = (int)(b0 & 0x07); }
            else return 0;
            if (pos + len > n) return 0;
            for (int k = 1; k < len; ++k) {
                const uint32_t b = s[pos + k];
                if ((b & 0xC0) != 0x80) return 0;
                cp = (cp << 6) | (int)(b & 0x3F);
            }
            const int need = cp <= 0x7F ? 1 : cp <= 0x7FF ? 2 : cp <= 0xFFFF ? 3 : cp <= 0x10FFFF ? 4 : 0;
            if (need != len || (cp & 0xFFFFF800) == 0xD800) return 0;            // shortest form only, no surrogates
        }
        cls[1 + nch] = (uint16_t)t.cp_pages[(uint32_t)t.cp_l1[cp >> 8] * 256u + (uint32_t)(cp & 255)];
        pos += len; ++nch;
    }
    if (nch == 0) return 0;                                                      // tokdll:847-849
    cls[0] = (uint16_t)t.cls_l; cls[nch + 1] = (uint16_t)t.cls_r;
    *src_bytes = (int)(pos - bom);
    return nch;
}

// the walk that starts at position `from` of a word's slot (FAHyphInterpreter_core_t.h:193-250).  or_slot(i, v): pattern value v lies on output slot i
BF_HD bool w2h_starts_at(const W2hTables &t, int nch, int from) { return from < nch + 2 - (t.min_pat_len - 1); }
template <class OrSlot>
BF_HD void w2h_walk(const W2hTables &t, const uint16_t *cls, int nch, int from, OrSlot &&or_slot)
{
    uint32_t state = t.initial;
    for (int i = from; i < nch + 2; ++i) {
        const uint32_t c = cls[i];
        const uint64_t e = t.T[state + c];
        if ((uint32_t)(e & T64_CLS_MASK) != c) break;
        state = (uint32_t)((e >> T64_NEXT_SHIFT) & T64_NEXT_MASK);
        if (!(e & T64_FINAL_BIT)) continue;
        const uint8_t *pat = t.pats + (uint32_t)(e >> T64_OW_SHIFT);
        const int len = (int)pat[0] | ((int)pat[1] << 8);
        int je = len;
        if (from + len - nch > 0) je -= from + len - nch;                        // clipped at the word's end
        for (int j = from == 0 ? 1 : 0; j < je; ++j) {                           // (the left anchor has no slot)
            const int v = pat[2 + j];
            if (v != HYPH_DONT_CARE) or_slot(from + j - 1, v);
        }
    }
}

// slot i of a word of nch characters, from the byte of values it saw: is a hyphen written behind character i?  (:226-263, tokdll:891-900)
BF_HD bool w2h_hyphen_after(const W2hTables &t, uint32_t seen, int i, int nch)
{
    const int nh = t.no_hyph_len < nch ? t.no_hyph_len : nch;
    if (i < nh) return false;
    const int k = nch - 2 - i;                                                   // the mirrored slot of the no-hyph fix-up
    if (i > 0 && k >= 0 && k < nh) return false;
    if (seen == 0 || (seen & (seen - 1)) != 0) return false;                     // HYPH_UNKNOWN / HYPH_CONFLICT
    return seen != 1u;                                                           // one value: above HYPH_NO_HYPH?
}

// the output of a word: its characters as decoded (U+0000 as U+0020), the hyphen's bytes behind every flagged one.  s: behind the BOM
template <class Put>
BF_HD void w2h_copy_word(const uint8_t *s, int nch, const uint16_t *flags, uint32_t hy_bytes, int hy_len, Put &&put)
{
    int pos = 0, o = 0;
    for (int i = 0; i < nch; ++i) {
        const uint32_t b0 = s[pos];
        const int len = b0 < 0x80 ? 1 : b0 < 0xE0 ? 2 : b0 < 0xF0 ? 3 : 4;
        if (len == 1) put(o++, (uint8_t)(b0 == 0 ? 0x20 : b0));
        else for (int k = 0; k < len; ++k) put(o++, s[pos + k]);
        pos += len;
        if (flags[i]) for (int k = 0; k < hy_len; ++k) put(o++, (uint8_t)(hy_bytes >> (8 * k)));
    }
}

// what the single call does with a word's complete output `full` of `need` bytes (tokdll:876-910): symbols are copied while they fit
// entirely, the count keeps running, a terminating 0 is written and counted only when there is room for it
inline int w2h_finish(const uint8_t *full, int need, char *out, int cap)
{
    if (out) {
        int pos = 0;
        while (pos < need) {
            const uint32_t b0 = full[pos];
            const int len = b0 < 0x80 ? 1 : b0 < 0xE0 ? 2 : b0 < 0xF0 ? 3 : 4;
            if (pos + len > cap) break;                                          // nothing behind it fits either: the count only grows
            for (int k = 0; k < len; ++k) out[pos + k] = (char)full[pos + k];
            pos += len;
        }
        if (need < cap) { out[need] = 0; return need + 1; }
    }
    return need;
}

// FAIntToUtf8 (FAUtf8Utils.cpp:471-527): bytes little end first; 0 = the reference refuses the symbol
inline int w2h_encode(int c, uint32_t *bytes)
{
    const uint32_t u = (uint32_t)c;
    if (u <= 0x7F) { *bytes = u; return 1; }
    if (u <= 0x7FF) { *bytes = (0xC0 | (u >> 6)) | ((0x80 | (u & 0x3F)) << 8); return 2; }
    if (u <= 0xFFFF) { if ((u & 0xFFFFF800u) == 0xD800u) return 0; *bytes = (0xE0 | (u >> 12)) | ((0x80 | ((u >> 6) & 0x3F)) << 8) | ((0x80 | (u & 0x3F)) << 16); return 3; }
    if (u <= 0x10FFFF) { *bytes = (0xF0 | (u >> 18)) | ((0x80 | ((u >> 12) & 0x3F)) << 8) | ((0x80 | ((u >> 6) & 0x3F)) << 16) | ((0x80u | (u & 0x3F)) << 24); return 4; }
    return 0;
}

} // namespace bfa
