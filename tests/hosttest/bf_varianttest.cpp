// bf_varianttest.cpp -- TEST-ONLY: the decode functions of blingfire_amd/csrc/bf_variant.h (the integer of BfSetVariant -> named knobs) and
// its table of the BPE wave program's instances behind a C interface, and nothing more (tests/test_variant_decode.py).
#include <stdint.h>
#include "../../blingfire_amd/csrc/bf_variant.h"

using namespace bfa;

extern "C" {

// the fields bft_variant_decode writes, in order, as "Struct.field" separated by commas
const char *bft_variant_fields()
{
    return "WpChoice.lane_only,WpChoice.flat_always,WpChoice.flat_by_size,WpWaveKnobs.grab,WpWaveKnobs.per_cu,"
           "WpFlatKnobs.per_cu,WpFlatKnobs.waves_per_simd,WpFlatKnobs.dbg,WpUnitsKnobs.per_cu,WpUnitsKnobs.cfg,"
           "LaneLexKnobs.ev_thresh,LaneLexKnobs.fetch_thresh,LaneLexKnobs.votes,LaneLexKnobs.per_cu,"
           "WordsKnobs.no_long,WordsKnobs.thresh_k,WordsKnobs.small_triples,WordsKnobs.chunks_40,WordsKnobs.two_level_from_256,"
           "SpPrepKnobs.old_form,SpPrepKnobs.waves,BpeWaveKnobs.off,BpeWaveKnobs.tune,BpeWaveKnobs.no_word_table,"
           "SegKnobs.per_doc_kernels,SegKnobs.no_local,SegKnobs.write_arcs,SegKnobs.cut_off,SegKnobs.cut_unroll2,SegKnobs.quick_or_one_kernel,"
           "SegKnobs.tune,SegKnobs.per_cu_cap";
}
enum { BFT_VARIANT_NFIELDS = 32 };

// out[i * 32 ..): every field of variant[i]; `words` is what the lane lexer is told (LaneLexKnobs is the only struct that depends on it)
void bft_variant_decode(const int32_t *variant, int64_t n, int words, int32_t *out)
{
    for (int64_t i = 0; i < n; ++i) {
        const int v = variant[i];
        const WpChoice c = wp_choice(v); const WpWaveKnobs w = wp_wave_knobs(v); const WpFlatKnobs f = wp_flat_knobs(v); const WpUnitsKnobs u = wp_units_knobs(v);
        const LaneLexKnobs l = lane_lex_knobs(v, words != 0); const WordsKnobs d = words_knobs(v); const SpPrepKnobs p = sp_prep_knobs(v);
        const BpeWaveKnobs b = bpe_wave_knobs(v); const SegKnobs g = seg_knobs(v);
        const int32_t row[BFT_VARIANT_NFIELDS] = {c.lane_only, c.flat_always, c.flat_by_size, w.grab, w.per_cu, f.per_cu, f.waves_per_simd, f.dbg, u.per_cu, u.cfg,
                                                  l.ev_thresh, l.fetch_thresh, l.votes, l.per_cu, d.no_long, d.thresh_k, d.small_triples, d.chunks_40, d.two_level_from_256,
                                                  p.old_form, p.waves, b.off, b.tune, b.no_word_table,
                                                  g.per_doc_kernels, g.no_local, g.write_arcs, g.cut_off, g.cut_unroll2, g.quick_or_one_kernel, g.tune, g.per_cu_cap};
        for (int k = 0; k < BFT_VARIANT_NFIELDS; ++k) out[i * BFT_VARIANT_NFIELDS + k] = row[k];
    }
}

void bft_variant_needs_experiments(const int32_t *variant, int64_t n, int wordpiece, int32_t *out)
{
    for (int64_t i = 0; i < n; ++i) out[i] = variant_needs_experiments(wordpiece != 0, variant[i]) ? 1 : 0;
}

// out = {steps, umin, home, experiments_only}: the table's own entry for `tune` / the instance a build runs for it
void bft_bpe_wave_entry(int tune, int32_t *out) { const BpeWaveTune t = BPE_WAVE_TUNES[tune & 15]; out[0] = t.steps; out[1] = t.umin; out[2] = t.home; out[3] = t.experiments_only; }
void bft_bpe_wave_tune(int tune, int experiments_build, int32_t *out) { const BpeWaveTune t = bpe_wave_tune(tune, experiments_build != 0); out[0] = t.steps; out[1] = t.umin; out[2] = t.home; out[3] = t.experiments_only; }
int bft_bpe_wave_home(int tune, int experiments_build) { return bpe_wave_home(tune, experiments_build != 0) ? 1 : 0; }

} // extern "C"
