// bf_variant.h -- the one place that knows the bit layout of the integer of BfSetVariant (bf_internal.h).  Host only, plain C++17.
//
// Handle::variant keeps the integer as the caller gave it; every reader decodes it here into a small struct of named knobs (bf_capi.cpp) and the
// launchers (bf_kernels.h) take those.  The integers themselves are a fixed interface: tests, tools and bench.py pass them hand-built.
//
//   bits    field                              read by (program)                                      0 means
//   ------  ---------------------------------  -----------------------------------------------------  ------------------------------------------
//   0..7    the low byte, as a whole number    WpChoice (WordPiece): 2 lane_only, 3 flat_by_size,     (3 is the default) any other value: the
//                                                4 flat_always                                          wave program, never the flat one
//                                              SegKnobs (BPE lane kernels): 2 per_doc_kernels,        the fused kernel with the lane-local solve
//                                                4 no_local, 5 write_arcs
//                                              SegKnobs (Unigram): 6 cut_off                          the cut form where it applies
//   4       0x10 cut_unroll2                   SegKnobs (Unigram cut form)                            three transitions per trip
//   5       0x20 quick_or_one_kernel           SegKnobs (Unigram: the cut form's quick flag; the      off
//                                                lane form's one-kernel instance, experiments builds)
//   6       0x40 off                           BpeWaveKnobs                                           the BPE wave program where the model admits it
//   7       0x80 old_form                      SpPrepKnobs                                            k_prep_sp8
//   8..11   cfg                                WpUnitsKnobs (k_wp_units instance)      [experiments]  shipped
//   8..11   tune                               BpeWaveKnobs (BPE_WAVE_TUNES below)                    shipped
//   8..15   ev_thresh                          LaneLexKnobs (8..11 only in the words modes)           32; 16 for two-level lexers
//   8..15   tune                               SegKnobs: vote threshold of k_bpe_fused, transitions   16 / 3 / a period of 32
//                                                per trip of the Unigram lane form [experiments],
//                                                period of the Unigram cut form
//   12..15  grab                               WpWaveKnobs: documents per grab                        by batch size
//   12..15  thresh_k                           WordsKnobs: long documents from 8 << k characters      total_bytes / 24,000, at least 16
//   16..19  waves_per_simd                     WpFlatKnobs (k_wp_flat instance)        [experiments]  shipped (7)
//   16..19  fetch_thresh                       LaneLexKnobs                            [experiments]  8
//   16..23  per_cu_cap                         SegKnobs: cap on the resident workgroups per CU        what fits
//   20..23  dbg                                WpFlatKnobs (WfParams::dbg)             [experiments]  off
//   20..23  votes                              LaneLexKnobs: transitions per vote      [experiments]  shipped (4)
//   20      0x100000 no_word_table             BpeWaveKnobs                                           the word table where the model has one
//   24..29  per_cu                             WpWaveKnobs, WpFlatKnobs, WpUnitsKnobs, LaneLexKnobs   what the occupancy query answers
//                                                (24..26 only in the words modes)
//   24..27  waves                              SpPrepKnobs (k_prep_sp8 instance)       [experiments]  the compiler's choice
//   27      0x08000000 two_level_from_256      WordsKnobs (test knob)                                 from 512 K cells
//   28      0x10000000 chunks_40               WordsKnobs (test knob)                                 LONG_MAX_CHUNKS
//   29      0x20000000 small_triples           WordsKnobs (test knob)                                 n triples
//   30      0x40000000 no_long                 WordsKnobs                                             the long-document path
//
// [experiments]: a non-zero value selects a measurement instance that only a BF_EXPERIMENTS build carries; BfSetVariant refuses it otherwise
// (variant_needs_experiments: by the handle's kind, since the same bits are plain tuning values for the other kind).
//
// Known overlaps, unchanged: the fields share bits because a handle runs one program at a time, but a WordPiece handle runs
// several.  Bits 12..15 are grab, the upper half of ev_thresh and thresh_k at once, so a words threshold set on a WordPiece handle also changes
// grab and ev_thresh of later TextToIds calls on it (the words modes themselves strip 12..15 and 27..30 before the lane lexer decodes); bits
// 8..11 are the units cfg and the lower half of ev_thresh; bits 24..29 are per_cu for four launchers and overlap the words knobs (27..30) and the
// prologue's waves (24..27); bits 16..23 are waves_per_simd + dbg, fetch_thresh + votes and per_cu_cap; 0x10 / 0x20 are part of the low byte the
// BPE lane kernels compare as a whole.
#pragma once

namespace bfa {

constexpr int variant_bits(int variant, int shift, int width) { return (int)(((unsigned)variant >> shift) & ((1u << width) - 1u)); }

struct WpChoice { bool lane_only, flat_always, flat_by_size; };
constexpr WpChoice wp_choice(int v) { return {variant_bits(v, 0, 8) == 2, variant_bits(v, 0, 8) == 4, variant_bits(v, 0, 8) == 3}; }

struct WpWaveKnobs { int grab, per_cu; };
constexpr WpWaveKnobs wp_wave_knobs(int v) { return {variant_bits(v, 12, 4), variant_bits(v, 24, 6)}; }

struct WpFlatKnobs { int per_cu, waves_per_simd, dbg; };
constexpr WpFlatKnobs wp_flat_knobs(int v) { return {variant_bits(v, 24, 6), variant_bits(v, 16, 4), variant_bits(v, 20, 4)}; }

struct WpUnitsKnobs { int per_cu, cfg; };
constexpr WpUnitsKnobs wp_units_knobs(int v) { return {variant_bits(v, 24, 6), variant_bits(v, 8, 4)}; }

// words modes: bits 12..15 are thresh_k and bits 27..30 the words knobs there, so the lane lexer sees neither
struct LaneLexKnobs { int ev_thresh, fetch_thresh, votes, per_cu; };
constexpr LaneLexKnobs lane_lex_knobs(int v, bool words) { return {variant_bits(v, 8, words ? 4 : 8), variant_bits(v, 16, 4), variant_bits(v, 20, 4), variant_bits(v, 24, words ? 3 : 6)}; }

struct WordsKnobs { bool no_long; int thresh_k; bool small_triples, chunks_40, two_level_from_256; };
constexpr WordsKnobs words_knobs(int v) { return {(v & 0x40000000) != 0, variant_bits(v, 12, 4), (v & 0x20000000) != 0, (v & 0x10000000) != 0, (v & 0x08000000) != 0}; }

struct SpPrepKnobs { bool old_form; int waves; };
constexpr SpPrepKnobs sp_prep_knobs(int v) { return {(v & 0x80) != 0, variant_bits(v, 24, 4)}; }

struct BpeWaveKnobs { bool off; int tune; bool no_word_table; };
constexpr BpeWaveKnobs bpe_wave_knobs(int v) { return {(v & 0x40) != 0, variant_bits(v, 8, 4), (v & 0x100000) != 0}; }

struct SegKnobs {
    bool per_doc_kernels, no_local, write_arcs;           // BPE
    bool cut_off, cut_unroll2, quick_or_one_kernel;       // Unigram
    int tune, per_cu_cap;
};
constexpr SegKnobs seg_knobs(int v)
{
    return {variant_bits(v, 0, 8) == 2, variant_bits(v, 0, 8) == 4, variant_bits(v, 0, 8) == 5,
            variant_bits(v, 0, 8) == 6, (v & 0x10) != 0, (v & 0x20) != 0, variant_bits(v, 8, 8), variant_bits(v, 16, 8)};
}

// the fields marked [experiments] above: 0x00FF0F00 on a WordPiece handle, 0x0F000000 on any other
constexpr bool variant_needs_experiments(bool wordpiece, int v)
{
    return wordpiece ? wp_units_knobs(v).cfg != 0 || wp_flat_knobs(v).waves_per_simd != 0 || wp_flat_knobs(v).dbg != 0 : sp_prep_knobs(v).waves != 0;
}

#ifdef BF_EXPERIMENTS
constexpr bool EXPERIMENTS_BUILD = true;
#else
constexpr bool EXPERIMENTS_BUILD = false;
#endif

// The instances of the BPE wave program (bf_bpe_wave_body.h) by BpeWaveKnobs::tune: transitions per round, the units phase ends with fewer than
// `umin` busy units, the HOME form (ids stay at their words' homes -> k_bpe_home_gather) or the in-order form of rounds 4..5 (ids retired through
// the queue -> k_compact_ids; 8 is what A/B runs and tests use).  A value without an instance in the build at hand runs the shipped one, [0].
struct BpeWaveTune { int steps, umin; bool home, experiments_only; };
constexpr BpeWaveTune BPE_WAVE_TUNES[16] = {
    {4, 32, true, false}, {4, 16, false, true}, {4, 4, false, true},  {4, 48, false, true}, {4, 32, true, false}, {4, 32, true, false}, {6, 32, false, true}, {4, 32, true, false},
    {4, 32, false, false}, {4, 48, true, false}, {3, 32, true, false}, {4, 60, true, false}, {4, 32, true, false}, {4, 32, true, false}, {4, 32, true, false},  {4, 32, true, false}};
constexpr BpeWaveTune bpe_wave_tune(int tune, bool experiments_build)
{
    return BPE_WAVE_TUNES[tune & 15].experiments_only && !experiments_build ? BPE_WAVE_TUNES[0] : BPE_WAVE_TUNES[tune & 15];
}
constexpr bool bpe_wave_home(int tune, bool experiments_build) { return bpe_wave_tune(tune, experiments_build).home; }

} // namespace bfa
