// bf_charpos.h -- byte offsets <-> character offsets (code points or UTF-16 code units) over text that is on the device.
//
// Additive (the reference has no counterpart; include/blingfiretokdll_amd.h ByteToCharOffsetsBatchDevice is the specification).  A byte has a
// weight (0 for a continuation byte, 2 for the lead of a four-byte character when the unit is UTF-16, else 1); C_d(i) is the weight of the first i
// bytes of document d, B_d(k) the first byte of the character that holds unit k.  The index is over the batch's text buffer in chunks of 64 bytes
// that ignore the documents: per chunk a mask of the bytes with a weight (and, for UTF-16, of the leads >= 0xF0), and P, the exclusive scan of the
// chunks' weights.  G(x) = P[x >> 6] + popcount(mask below x & 63) is the weight of text[0, x), C_d(i) = G(off_d + i) - G(off_d), and B_d is a
// search of P over the document's chunks followed by a bisection inside one chunk's masks.  Everything is 64-bit: a batch holds more than 2^31 bytes.
//
// Everything a lane decides is written once here as BF_HD code: bf_kernels_charpos.hip runs it per lane, tests/hosttest compiles the same header
// for the host (test-only: the product library never converts offsets on the CPU).  Plain C++, no HIP types.
#pragma once
#include <stdint.h>
#include "bf_rows.h"

namespace bfa {

constexpr int CHARPOS_CHUNK = 64;                 // bytes a mask covers: one bit per byte
constexpr int CHARPOS_LANE_BYTES = 16;            // bytes a lane of k_char_index takes: four lanes make a chunk, a wave 16 chunks
constexpr int CHARPOS_WAVE_BYTES = 64 * CHARPOS_LANE_BYTES;
constexpr int CHARPOS_UNIT_CHAR = 0, CHARPOS_UNIT_UTF16 = 1;
constexpr int CHARPOS_ENDS_IN_EXCLUSIVE = 1;      // flags bit 0
constexpr int CHARPOS_ENDS_OUT_EXCLUSIVE = 2;     // flags bit 1
constexpr int CHARPOS_FLAGS = 3;
constexpr int CHARPOS_FWD = 0, CHARPOS_INV = 1;   // bytes -> units, units -> bytes

BF_HD int64_t charpos_nchunks(int64_t total_bytes) { return (total_bytes + CHARPOS_CHUNK - 1) / CHARPOS_CHUNK; }

BF_HD int charpos_popc(uint64_t m) { return __builtin_popcountll(m); }

// the bits below bit r, r = 0 .. 64
BF_HD uint64_t charpos_low(int r) { return r >= 64 ? ~(uint64_t)0 : (((uint64_t)1 << r) - 1); }

// ---- the index pass.  Four bytes as one little-endian word -> four bits each: byte k has a weight (it is no continuation byte) / is >= 0xF0.
// A continuation byte has bit 7 set and bit 6 clear; the four flags at bits 7, 15, 23, 31 are gathered by one multiplication (the sixteen
// partial products land on sixteen different bits: nothing carries).
BF_HD uint32_t charpos_gather4(uint32_t at_bit7) { return (((at_bit7 >> 7) * 0x00204081u) >> 21) & 0xFu; }
BF_HD uint32_t charpos_lead4(uint32_t w) { return charpos_gather4(~(w & ~(w << 1)) & 0x80808080u); }
BF_HD uint32_t charpos_four4(uint32_t w) { return charpos_gather4(w & (w << 1) & (w << 2) & (w << 3) & 0x80808080u); }

// a lane's sixteen bytes (four words) -> its sixteen-bit pieces of the two masks
BF_HD void charpos_piece(const uint32_t w[4], uint32_t *lead16, uint32_t *four16)
{
    *lead16 = charpos_lead4(w[0]) | (charpos_lead4(w[1]) << 4) | (charpos_lead4(w[2]) << 8) | (charpos_lead4(w[3]) << 12);
    *four16 = charpos_four4(w[0]) | (charpos_four4(w[1]) << 4) | (charpos_four4(w[2]) << 8) | (charpos_four4(w[3]) << 12);
}

// the sixteen bytes at `at` of a text of `total` bytes, for the lane that holds the text's end: a byte at or past the end reads as a
// continuation byte (0x80) and is not loaded
BF_HD void charpos_tail_words(const uint8_t *text, int64_t at, int64_t total, uint32_t w[4])
{
    for (int k = 0; k < 4; ++k) {
        uint32_t x = 0;
        for (int j = 0; j < 4; ++j) {
            const int64_t i = at + 4 * k + j;
            x |= (uint32_t)(i < total ? text[i] : (uint8_t)0x80) << (8 * j);
        }
        w[k] = x;
    }
}

// where a lane's piece stands in its chunk's mask (lane & 3 = the quarter)
BF_HD uint64_t charpos_place(uint32_t piece16, int lane) { return (uint64_t)piece16 << (16 * (lane & 3)); }

// the weight of a chunk from its finished masks (four == 0 for code points)
BF_HD int32_t charpos_chunk_count(uint64_t lead, uint64_t four) { return charpos_popc(lead) + charpos_popc(four); }

// ---- the index as the convert kernels read it: four == nullptr for code points
struct CharIndex { const uint64_t *lead, *four; const int64_t *P; };

// the weight of chunk c's bytes below r (0 .. 64), from masks a lane holds
BF_HD int charpos_below(uint64_t lead, uint64_t four, int r) { const uint64_t m = charpos_low(r); return charpos_popc(lead & m) + charpos_popc(four & m); }

// G(x), 0 <= x <= total_bytes: the weight of text[0, x).  On a chunk edge P alone answers (x = total_bytes on an edge has no chunk to load)
BF_HD int64_t charpos_G(const CharIndex &ix, int64_t x)
{
    const int64_t c = x >> 6;
    const int r = (int)(x & 63);
    if (r == 0) return ix.P[c];
    return ix.P[c] + charpos_below(ix.lead[c], ix.four ? ix.four[c] : 0, r);
}

// a document as the kernels see it: n = 0 where its range is not inside [0, total_bytes] or its offsets decrease (bad; status bit 3)
struct CharDoc { int64_t b, n; bool bad; };
BF_HD CharDoc charpos_doc(int64_t b, int64_t e, int64_t total_bytes)
{
    CharDoc d;
    d.n = rows_seq_len(b, e, total_bytes, &d.bad);
    d.b = d.bad ? 0 : b;
    return d;
}

// U_d
BF_HD int64_t charpos_units(const CharIndex &ix, const CharDoc &d) { return d.n > 0 ? charpos_G(ix, d.b + d.n) - charpos_G(ix, d.b) : 0; }

// the document of item i: the last d in [lo, hi] with off[d] <= i (off[lo] <= i holds; hi < ndocs), one lane's binary search
BF_HD int64_t charpos_item_doc(const int64_t *off, int64_t lo, int64_t hi, int64_t i)
{
    ++hi;
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (off[mid] <= i) lo = mid; else hi = mid;
    }
    return lo;
}

// B_d(k) for 0 <= k < U: the byte, relative to the document, of the character that holds unit k.  Gb = G(d.b).  The chunk is the last one of the
// document's with P <= Gb + k (the document's first chunk qualifies: P of it <= Gb); inside it the weight below r is monotone in r, and
// the byte wanted is the r with below(r) <= t < below(r + 1): six halvings of [0, 64].  The answer lies inside the document: the weight in
// front of d.b is <= Gb + k, and k < U leaves a byte with a weight in front of the document's end.
BF_HD int64_t charpos_unit_byte(const CharIndex &ix, const CharDoc &d, int64_t Gb, int64_t k)
{
    const int64_t T = Gb + k;
    int64_t lo = d.b >> 6, hi = ((d.b + d.n - 1) >> 6) + 1;
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (ix.P[mid] <= T) lo = mid; else hi = mid;
    }
    const int t = (int)(T - ix.P[lo]);
    const uint64_t lead = ix.lead[lo], four = ix.four ? ix.four[lo] : 0;
    int rl = 0, rh = 64;
    while (rh - rl > 1) {
        const int mid = (rl + rh) >> 1;
        if (charpos_below(lead, four, mid) <= t) rl = mid; else rh = mid;
    }
    return lo * 64 + rl - d.b;
}

// F(x) of the specification: C_d(x) (dir = CHARPOS_FWD, limit = n_d) or B_d(x) (CHARPOS_INV, limit = U_d) for 0 <= x; -1 and *bad where x is
// beyond the limit or the answer beyond INT32_MAX
BF_HD int64_t charpos_F(const CharIndex &ix, const CharDoc &d, int64_t Gb, int64_t U, int dir, int64_t x, bool *bad)
{
    const int64_t limit = dir == CHARPOS_FWD ? d.n : U;
    if (x > limit) { *bad = true; return -1; }
    int64_t y;
    if (dir == CHARPOS_FWD) y = x == 0 ? 0 : charpos_G(ix, d.b + x) - Gb;
    else y = x == U ? d.n : charpos_unit_byte(ix, d, Gb, x);
    if (y > 0x7fffffff) { *bad = true; return -1; }
    return y;
}

// one start (is_end = false) or one end of an item: a negative input gives -1 and no status bit
BF_HD int32_t charpos_convert(const CharIndex &ix, const CharDoc &d, int64_t Gb, int64_t U, int dir, int flags, bool is_end, int32_t v, bool *bad)
{
    if (v < 0) return -1;
    int64_t x = v;
    if (is_end && !(flags & CHARPOS_ENDS_IN_EXCLUSIVE)) x += 1;
    const int64_t y = charpos_F(ix, d, Gb, U, dir, x, bad);
    if (y < 0) return -1;
    return (int32_t)(is_end && !(flags & CHARPOS_ENDS_OUT_EXCLUSIVE) ? y - 1 : y);
}

// U_d as the int32 d_doc_units_out holds: a document of more units saturates
BF_HD int32_t charpos_units32(int64_t U) { return U > 0x7fffffff ? 0x7fffffff : (int32_t)U; }

} // namespace bfa
