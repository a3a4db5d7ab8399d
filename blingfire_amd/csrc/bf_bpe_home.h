// bf_bpe_home.h -- the spans of the HOME form of the BPE wave program (bf_bpe_wave_body.h, SPANS instance): what k_bpe_home_spans
// (bf_kernels_sp.hip) does with one block of 64 staging cells, shared with the host test (tests/hosttest/bf_bpeoffstest.cpp).
//
// The SPANS instance leaves every id in the cell under its piece's first stream element.  Pieces tile their word and words tile the document, so
//   from = the id's cell index,   to = the next id cell - 1, or L - 1 behind the document's last id.
// A block of 64 cells is one 64-bit mask (bit = the cell holds an id).  A piece is no longer than its word, a word no longer than BH_PIECE_MAX
// elements: the next id cell of a cell of block b lies in block b or in block b + 1, or nowhere -- one mask of look-ahead.
// Stream positions become byte offsets by k_compact's rule (tokdll:1270-1272,1527-1528): the element -> source byte stream of the prologue at
// both ends, the end moved to the last byte of the character that starts there; -1 stays -1 (the dummy prefix has no source byte).
#pragma once
#include <stdint.h>

#if !defined(BF_HD)
#if defined(__HIPCC__)
#define BF_HD __host__ __device__ __forceinline__
#else
#define BF_HD inline
#endif
#endif

namespace bfa {

constexpr int BH_BLOCK = 64;
constexpr int BH_PIECE_MAX = BH_BLOCK;      // the look-ahead of one mask holds for pieces of at most this many elements (the users assert BW_WORD_MAX against it)

// The next id cell behind cell `lane` of a block: `own` = the block's mask, `ahead` = the following block's.  Returns its distance from the
// block's first cell (1 .. 127), or -1: no id cell in either.
BF_HD int bh_next_cell(unsigned long long own, unsigned long long ahead, int lane)
{
    const unsigned long long above = lane < 63 ? own >> (lane + 1) : 0ull;
    if (above) return lane + 1 + __builtin_ctzll(above);
    if (ahead) return BH_BLOCK + __builtin_ctzll(ahead);
    return -1;
}

// [from, to] of the id in cell `lane` of the block that starts at cell `base` of a document of L elements
BF_HD void bh_span(unsigned long long own, unsigned long long ahead, int base, int lane, int L, int &from, int &to)
{
    const int nx = bh_next_cell(own, ahead, lane);
    from = base + lane;
    to = nx < 0 ? L - 1 : base + nx - 1;
}

// stream positions -> [first byte, last byte] in the document's text (src_off, text: the document's own)
BF_HD void bh_bytes(const int32_t *src_off, const uint8_t *text, int from, int to, int &first, int &last)
{
    first = from >= 0 ? src_off[from] : -1;
    const int eo = to >= 0 ? src_off[to] : -1;
    int sz = 0;
    if (eo >= 0) { const uint32_t ch = text[eo]; sz = (ch & 0x80) == 0 ? 1 : (ch & 0xE0) == 0xC0 ? 2 : (ch & 0xF0) == 0xE0 ? 3 : (ch & 0xF8) == 0xF0 ? 4 : 0; }
    last = eo + (sz > 0 ? sz - 1 : 0);
}

} // namespace bfa
