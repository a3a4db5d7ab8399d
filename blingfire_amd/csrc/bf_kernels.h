// bf_kernels.h -- device-side parameter blocks + launch wrappers (implemented in the bf_kernels*.hip units).
#pragma once
#include <stdint.h>
#include <hip/hip_runtime_api.h>
#include "bf_lex.h"
#include "bf_seg.h"
#include "bf_batch.h"
#include "bf_wave.h"
#include "bf_bpe_wave.h"
#include "bf_flat.h"
#include "bf_w2h.h"
#include "bf_rows.h"
#include "bf_pairs.h"
#include "bf_packed.h"
#include "bf_stream.h"
#include "bf_mlm.h"
#include "bf_denoise.h"
#include "bf_charpos.h"
#include "bf_variant.h"

namespace bfa {

struct WpPrepParams {
    Batch b;
    DevCpMap cpmap;             // fused charmap+class map (bf_model.h Model::wbd_cpmap)
    const uint16_t *multi_pool; // records for 0 / 2..10 output chars
    int has_multi;
    uint16_t *cls;              // [total_bytes] class stream: document d occupies cls[doc_off[d] ..)
    int32_t *src_off;           // optional (offsets API): byte offset in the document of the source character of every stream element
    int32_t *nchars;            // [ndocs] normalised length, 0 = "TextToIds returns 0"
    // optional (k_prep_wp, the one-pass form): documents of more than PREP_LONG_BYTES bytes are listed here and decoded by sixteen waves
    // each (k_prep_wp_long) instead of one; long_count is zeroed per launch
    int64_t *long_list; unsigned int *long_count; int64_t long_cap;
};

// Long documents of the words modes (bf_lex.h: lex_one_start / lex_chain_visit).  A document of more than `thresh` characters is
// listed (k_lex_long_list) and leaves the lane kernel alone; its n + 1 start positions are cells of a dense "chunk space" (64 cells
// per chunk, a document owns whole chunks: cell = 64 * chunk0 + position + 1) that three kernels go over:
//   k_lex_long<false>   every cell runs its start position without output (spec), then the wave resolves its own chunk: from every cell,
//                       the first cell beyond the chunk the chain reaches and the counts summed on the way there (jump);
//   k_lex_long_chain    one workgroup per document goes from chunk to chunk, one hop each: where the chain enters a chunk and the
//                       output index / triples so far at that point (entry);
//   k_lex_long<true>    every entered chunk follows the chain inside itself, the visited cells run again and write their tokens into
//                       the document's staging slot.
struct LexLongDoc { int64_t doc, chunk0; };       // doc < 0: a listed document that did not fit the workspace (the lane kernel keeps it)
struct LexLongParams {
    int thresh;                       // 0: off
    int cap_shift;                    // test knob (BfSetVariant 0x20000000): the triple buffer holds n >> cap_shift triples instead of n (lane kernel too)
    int64_t cap_docs, cap_chunks;     // capacity of `list` / of the cell arrays in chunks
    unsigned long long *hdr;          // documents listed << 32 | chunks handed out (zeroed per launch)
    LexLongDoc *list;
    int32_t *spec;                    // [4 * cell]: next position, tokens output, triples produced, tag of the first token
    int32_t *jump;                    // [4 * cell]: first cell of the document beyond this chunk on the chain from here (LEX_CHAIN_END: none), tokens / triples summed up to there,
                                      // the span of the position's first token when it writes one or two (0x80000000 | first - position << 16 | last - position; else 0):
                                      // those are written without a second walk
    int32_t *tok2;                    // [2 * cell]: tag and span of the second token of a position that writes two (the span of the first in `jump` is 0 unless both pack)
    // documents of more than `big_cells` cells (0: none) take the chain in two levels: jump2 = the same as jump for the document's
    // 64-chunk super-chunks (k_lex_long_jump2), entry2[first chunk of a super-chunk] = the CELL OF THE DOCUMENT the chain enters it at
    // (-1: it does not), tokens / triples before it (k_lex_long_chain2); k_lex_long_chain3 fills `entry` per super-chunk
    int big_cells;
    int32_t *jump2;                   // [4 * cell]
    int32_t *entry2;                  // [4 * chunk] (used at the first chunk of every super-chunk)
    int32_t *entry;                   // [4 * chunk]: cell of the chunk the chain enters at (-1: it does not), tokens output / triples produced before it, -
};
constexpr int LEX_CHAIN_END = 0x40000000, LEX_COUNT_SAT = 0x3fffffff;
constexpr unsigned long long LEX_LONG_CHUNK_MASK = (1ull << 32) - 1;

struct WpLexParams {
    LexTables L;
    Batch b;
    const uint16_t *cls;
    const int32_t *nchars;
    int32_t *ids_tmp;           // [total_bytes] staging: document d writes ids_tmp[doc_off[d] ..)
    int32_t *span_tmp;          // optional (offsets API): [2k],[2k+1] = first / last stream position of staged id k
    int32_t *counts;            // [ndocs]
    int max_ids, unk;
    unsigned long long *next_doc; // work counter (persistent variants)
    int *status;
    int ev_thresh, fetch_thresh;  // vote thresholds of the divergence-aware driver
    int acts_n;                   // ints in L.acts (staged in LDS when small)
    int words;                    // TextToWords mode (bf_lex.h LexLane::words)
    unsigned long long *stats;    // optional instrumentation counters (experiments), else nullptr
    int table_n;                  // entries of L.T that can hold a transition (the branch-free probe tail behind them is all empty):
                                  // when they fit, the kernel stages them in LDS (bf_kernels.hip TabLds)
    LexLongParams lg;             // words modes: the long-document path (thresh 0 = every document on a lane)
};

// _sp branch: element slot of document d (stream, DP arrays and the id staging slot share it):
//   first element = slot_mul * (doc_off[d] + d), capacity slot_mul * (nbytes + 1)
struct SpPrepParams {
    Batch b;
    DevCpMap cpmap;             // fused charmap + element-code map (bf_model.h Model::sp_cpmap)
    const uint16_t *multi_pool;
    int has_multi, use_bytes, has_charmap;
    uint16_t delim_code;
    int prefix_n; uint16_t prefix[10];
    int slot_mul;
    uint16_t *stream;           // element codes after prefix / charmap / whitespace collapse
    int32_t *src_off;           // optional (offsets API): byte offset of the source character of every kept element (-1: dummy prefix)
    int32_t *lens;              // [ndocs] stream length, 0 = "TextToIds returns 0"
    int old_form;               // experiments: the byte-per-lane kernel
    int waves;                  // experiments: waves per SIMD the eight-bytes-per-lane kernel is compiled for (0 = the compiler's choice)
};

struct SpSegParams {
    SegTables S;
    Batch b;
    const uint16_t *stream; const int32_t *lens;
    int slot_mul;
    int32_t *ids_tmp; int32_t *counts;
    int32_t *span_tmp;          // optional (offsets API)
    int max_ids, unk;
    // scratch (indexed by element slot): unigram sc/bi; bpe arcs (6 per element + 32 per document), tos/idsv/inter
    SegBest *best;
    SegArc *arcs; int32_t *tos; int32_t *idsv; uint8_t *inter;
    int *status;
    // documents are handed to lanes in order of stream length (counting sort), so the 64 documents of a wave
    // are of similar size: perm[i] = document processed by thread i; hist = 1024 bucket counters / cursors
    int32_t *perm; unsigned int *hist;
    int32_t *narcs;             // [ndocs] BPE arc count per document (-1 = capacity exceeded); Unigram: first id index within the slot
    int trie_depth;             // longest dictionary entry (bounds every arc length)
    int lane_ok;                // Unigram: the model fits the lane program (bf_seg.h UniLane: entries <= 32 symbols, ids < 2^20 - 2)
    int uni_cut = 0;            // Unigram: the cut form (bf_seg.h UniCut; ids only): tokens leave as words (bf_seg.h: key / symbols to walk / unknown), left-aligned in the slot -> k_uni_ids
    int64_t bm_words;           // BPE apply: words per bitmap (the two bitmaps live in the `tos` buffer)
    int32_t *fb_list; unsigned int *fb_count;   // BPE: documents k_bpe_fused hands to the full path (set by launch_seg_sp)
    uint8_t *big_pool; unsigned long long big_cap; unsigned long long *big_used, *big_need;   // BPE: pool of the documents whose arcs exceed the per-document reserve (k_bpe_seg); *big_need: bytes that did not fit
    const uint32_t *bpe_prio; const int32_t *bpe_place_id; uint32_t bpe_unk_prio; int bpe_prio_bits;   // bf_bpe_seg_body.h: the arc order as integers (bf_model.h)
    unsigned long long *seg_stats;   // optional (experiments): counters of k_bpe_seg
    int tune;                   // SegKnobs::tune, here because k_bpe_fused reads it on the device: the vote threshold of its lane-local solve (p.tune ? p.tune : 16)
    unsigned long long *next_doc;
    void *ev_dom0 = nullptr, *ev_dom1 = nullptr;   // optional (hipEvent_t): recorded around the dominant kernel of the step (the Unigram forward pass)
};

// key -> info lookup (reference FADictInterpreter_t<int>::GetInfo) for a batch of keys: key k = keys[key_off[k] .. key_off[k+1])
struct DictParams {
    DictTables D;
    const int32_t *rows; int stride, min_key, nrows;          // I2Info rows: [count or -1, values...]
    const int32_t *keys; const int64_t *key_off; int64_t nkeys;
    int32_t *info_ids;            // [nkeys] GetInfoId
    int32_t *ret;                 // [nkeys] GetInfo return value: value count, -1 = no such key / row
    int32_t *counts;              // [nkeys] values written for the key (max(ret, 0)) -> scanned into val_off
    const int64_t *val_off; int32_t *vals; int64_t vals_cap;
};
void launch_dict_ids(const DictParams &p, hipStream_t s);
void launch_dict_fill(const DictParams &p, hipStream_t s);

// the ids of the tokens of the Unigram cut form, written to their place in the caller's array (bf_kernels_sp.hip k_uni_ids)
struct UniIdsParams {
    Batch b; const uint64_t *T; uint32_t initial; const int32_t *ids;     // dictionary transitions; the id column of I2Info
    const uint16_t *stream; const int32_t *lens; int slot_mul;
    const int32_t *toks; const int32_t *counts; const int64_t *id_off;
    int32_t *ids_out; int64_t ids_cap; int unk, id_offset; int *status;
};
void launch_uni_ids(const UniIdsParams &p, hipStream_t s);

// the HOME form of the BPE wave program (bf_bpe_wave_body.h): ids at their words' homes -> counts -> (scan) -> the caller's array (bf_kernels_sp.hip)
struct BpeHomeParams {
    Batch b; const int32_t *ids_tmp; const int32_t *lens; const int32_t *flags; int slot_mul;
    int32_t *counts; const int64_t *id_off; int32_t *ids_out; int64_t ids_cap; int max_ids; int *status;
};
void launch_bpe_home_gather(const BpeHomeParams &p, hipStream_t s);

struct ScanParams { const int32_t *counts; int64_t ndocs; int64_t *id_off; int64_t *block_sums; int nblocks; };

struct CompactParams {
    Batch b; const int32_t *ids_tmp; const int32_t *counts; const int64_t *id_off;
    int32_t *ids_out; int64_t ids_cap; int *status;
    int slot_mul;               // 0: _wp slots (align8(doc_off)+8d); >0: _sp slots (slot_mul*(doc_off+d))
    const int32_t *first;       // optional: index of the first id inside the slot (Unigram flat kernel writes ids right-aligned)
    // offsets API (all optional): stream positions of the staged ids -> byte offsets in the original text (tokdll:1263-1273,1519-1529)
    const int32_t *span_tmp; const int32_t *src_off; int32_t *starts_out; int32_t *ends_out;
    const unsigned int *only_if = nullptr;      // optional: nothing to do when *only_if == 0 (the documents the flat program hands back: usually none)
};

// flags: one bit per 16-byte chunk of the text (u64 per KiB, + 1), or nullptr for the one-pass wave-per-document form
void launch_prep_wp(const WpPrepParams &p, int64_t total_bytes, unsigned long long *flags, hipStream_t s);
void launch_lex_wp(const WpLexParams &p, const LaneLexKnobs &k, hipStream_t s);
void launch_lex_long_list(const WpLexParams &p, hipStream_t s);      // before launch_lex_wp: lists the long documents (counts[doc] = -1)
void launch_lex_long(const WpLexParams &p, hipStream_t s);           // after it: the three kernels of the long-document path
void launch_wp_wave(const WpWaveParams &p, const WpWaveKnobs &k, hipStream_t s);     // unit-form lexers (bf_wave.h): replaces prep + lexer
// the flat program (bf_flat.h): ranges + fitness of the batch, the program, the documents it hands back, counts, merge
int wp_flat_ranges(int64_t ndocs, int64_t total_bytes);
void launch_wp_pre(const int64_t *doc_off, int64_t ndocs, int64_t total_bytes, int nranges, int64_t *range_doc, int *unsafe, hipStream_t s);
void launch_wp_flat(const WfParams &p, const WpFlatKnobs &k, hipStream_t s);
void launch_wp_units(const WfUnitParams &p, const WpUnitsKnobs &k, hipStream_t s);
void launch_wp_hardlist(const int32_t *dstat, const int *unsafe, int64_t ndocs, int32_t *list, unsigned int *list_n, hipStream_t s);
void launch_wp_count(const WfMergeParams &p, hipStream_t s);
void launch_wp_merge(const WfMergeParams &p, hipStream_t s);
void launch_bpe_wave(const BpeWaveParams &p, int tune, hipStream_t s);                  // bpe-opt models (bf_bpe_wave_body.h); tune: bf_variant.h BPE_WAVE_TUNES
void launch_bpe_seg_flags(const SpSegParams &p, const int32_t *flags, int32_t *list, unsigned int *count, hipStream_t s);   // the documents it hands back: bf_bpe_seg_body.h
void launch_prep_sp(const SpPrepParams &p, hipStream_t s);
void launch_seg_sp(const SpSegParams &p, const SegKnobs &k, hipStream_t s);
void launch_scan(const ScanParams &p, hipStream_t s);

// IdsToText (reference tokdll:1689-1745) as a batch: ids of sequence d are ids[id_off[d] .. id_off[d+1])
struct I2tParams {
    const uint32_t *tok_off; const uint8_t *tok_data; int ntok;   // [i2w] string array
    int min_id, max_id, skip_special;
    const int32_t *ids; const int64_t *id_off; int64_t nseq;
    int32_t *lens;               // [nseq] bytes of text per sequence (no terminator); 0 for an empty / failed sequence
    const int64_t *text_off;     // [nseq + 1] exclusive scan of lens (copy pass)
    uint8_t *text; int64_t text_cap;
    int *status;                 // bit 2: a sequence contains an id the model does not know (the reference returns 0 for it)
};
void launch_i2t_len(const I2tParams &p, hipStream_t s);

// TextToWords output assembly as a batch (reference tokdll:502-565): words of document d = spans word_off[d] .. word_off[d+1]
// (byte offsets relative to the document), joined by ' ', a ' ' or NUL inside a word written as '_'
struct W2tParams {
    const uint8_t *text; const int64_t *doc_off; int64_t ndocs;
    const int64_t *word_off; const int32_t *starts, *ends;
    int32_t *lens; const int64_t *text_off; uint8_t *out; int64_t out_cap;
    const int32_t *nvalid;       // sentences only: characters decoded per document (<= 0: the document is rejected)
    // optional (the copy kernels): documents of more than W2T_LONG_TOKENS tokens are listed here and assembled by sixteen waves each
    // (k_w2t_copy_long); long_count is zeroed by the caller
    int64_t *long_list; unsigned int *long_count; int64_t long_cap;
};
void launch_w2t_len(const W2tParams &p, hipStream_t s);
// TextToSentences output assembly (reference tokdll:257-339) on the same parameters: ends[] = last byte of every token of the
// sentence breaker (starts[] unused); a sentence runs from the byte after the previous token to the token's last byte, the rest
// of the document is the last sentence; leading white space dropped, '\n' / NUL -> ' ', sentences joined by '\n'
void launch_s2t_len(const W2tParams &p, hipStream_t s);
void launch_s2t_copy(const W2tParams &p, hipStream_t s);
void launch_w2t_copy(const W2tParams &p, hipStream_t s);

// NormalizeSpaces (reference tokdll:629-679) and TextToHashes (tokdll:683-815) as batches; both are model-free
struct NormSpParams {
    const uint8_t *text; const int64_t *doc_off; int64_t ndocs;
    int u_space, usp_len; uint32_t usp_bytes;   // uSpace, its UTF-8 length (0 if it cannot be encoded) and bytes (little end first)
    int32_t *lens;               // [ndocs] output bytes (0 on error)
    int32_t *aux;                // [ndocs] bit 0: error (empty / invalid UTF-8); bits 1..: normalised spaces left after the trim (saturating)
    const int64_t *out_off; uint8_t *out; int64_t out_cap;      // write pass
};
void launch_normsp(const NormSpParams &p, bool write, hipStream_t s);
struct HashParams {
    const uint8_t *text; const int64_t *doc_off; int64_t ndocs;
    int ngrams, bucket;
    int32_t *lens;               // [ndocs] (spaces + 1) * ngrams
    const int64_t *out_off; int32_t *out; int64_t out_cap;
};
void launch_hash_count(const HashParams &p, hipStream_t s);
void launch_hash_fill(const HashParams &p, hipStream_t s);
void launch_i2t_copy(const I2tParams &p, hipStream_t s);

// WordHyphenation (reference tokdll:818-911, FAHyphInterpreter_core_t.h:136-267) as a batch: word w = text[word_off[w] .. word_off[w+1]); bf_w2h.h, bf_kernels_w2h.hip
struct W2hParams {
    W2hTables t;
    const uint8_t *text; const int64_t *word_off; int64_t nwords, total_bytes; int *status;
    uint16_t *cls;               // position stream, [total_bytes + 2 * nwords]: classes, then the "a hyphen follows" flags (bf_w2h.h w2h_slot)
    int32_t *nch, *srcb;         // [nwords] characters (0: the word yields nothing) and the bytes they take in the source
    int32_t *lens;               // [nwords] output bytes (no terminator)
    int hy_len; uint32_t hy_bytes;      // the hyphen's UTF-8 length (1 .. 4) and bytes, little end first
    const int64_t *out_off; uint8_t *out; int64_t out_cap;      // copy pass
};
void launch_w2h_prep(const W2hParams &p, hipStream_t s);
void launch_w2h_walk(const W2hParams &p, hipStream_t s);
void launch_w2h_copy(const W2hParams &p, hipStream_t s);

// IdsToRowsBatch / IdsToPairRowsBatch (additive): items of a source S (bf_rows.h RowsSource: ragged ids; bf_pairs.h PairsSource: pairs of them) ->
// rows of row_len cells + mask (+ type where S has one).  The kernels are bf_rowstage_body.h, instantiated for RowsSource in bf_kernels_rows.hip and
// for PairsSource in bf_kernels_pairs.hip.
template <class S>
struct RowStageParams {
    S src;
    int64_t nseq; int *status;
    int32_t *counts;             // [nseq] rows per item
    const int64_t *row_off;      // [nseq + 1] exclusive scan of counts; row_off[nseq] = the row total, read on the device
    int64_t rows_cap;            // no row r >= rows_cap of any output is written
    int32_t *rows; uint8_t *mask;                                    // [rows_cap * row_len] each, either may be NULL
    // item and first id of every row: the caller's arrays (seq_rows / first_rows = rows_cap) or, for one the caller left out, the
    // handle's workspace and the rows it holds; the fill finds a row at or past them by its own search
    int32_t *row_seq, *row_first; int64_t seq_rows, first_rows;
    // [rows_cap * row_len] like mask, may be NULL (always, where S has none).  Last, so that a source without one leaves the kernel arguments it
    // reads where they were: the RowsSource kernels then have the instruction counts of the hand-written ones, with it behind `mask` two more
    uint8_t *type;
};
template <class S> void launch_rowstage_count(const RowStageParams<S> &p, hipStream_t s);
template <class S> void launch_rowstage_map(const RowStageParams<S> &p, hipStream_t s);
template <class S> void launch_rowstage_fill(const RowStageParams<S> &p, hipStream_t s);
// IdsToRowsPlanesBatch / IdsToPairRowsPlanesBatch (additive): up to ROWS_MAX_PLANES int32 arrays parallel to the ids, gathered into planes with the
// layout of `rows` by k_rowstage_planes (bf_rowstage_body.h), behind the map (and the fill) of the same call.  A struct of its own: the three
// kernels above keep their arguments where they are.
constexpr int ROWS_MAX_PLANES = 4;
template <class S>
struct RowPlanesParams {
    RowStageParams<S> st;        // the call's row stage as its kernels saw it: source, row offsets, capacity, a row's item and first id
    int nplanes;
    const int32_t *src[2][ROWS_MAX_PLANES];      // [side][k] (bf_rows.h CELL_SIDE_A / CELL_SIDE_B): parallel to the ids of that side (RowsSource: side 0 alone); NULL = that side's cells take the fill
    int32_t fill[ROWS_MAX_PLANES];               // what a cell without an id gets
    int32_t *out[ROWS_MAX_PLANES];               // [rows_cap * row_len] each; NULL = not taken
};
template <class S> void launch_rowstage_planes(const RowPlanesParams<S> &p, hipStream_t s);

// RowsSpanCellsBatchDevice (additive; bf_rows.h span_*, k_rows_span in bf_kernels_rows.hip): the cells of every row that hold the two ends of its item's byte span
struct RowsSpanParams {
    const int32_t *start_plane, *end_plane; int row_len;
    int64_t rows_cap; const int64_t *nrows;      // rows below min(rows_cap, *nrows); nrows NULL = rows_cap
    const int32_t *row_seq; int64_t nseq;        // a row's item (NULL: row r is item r); an item outside [0, nseq) has no span (status bit 3)
    const int32_t *span_first, *span_last; int none_cell;
    int32_t *start_cell, *end_cell; int *status;
};
void launch_rows_span(const RowsSpanParams &p, hipStream_t s);
unsigned rows_blocks(int64_t items);      // blocks of 256 lanes for `items` lanes, a grid-stride loop beyond 8 blocks per CU (bf_kernels_rows.hip)

// RowsMlmMaskBatchDevice (additive; bf_mlm.h has the lane code, k_rows_mlm in bf_kernels_mlm.hip): masked ids and labels of rows that are already there
struct RowsMlmParams {
    const int32_t *rows; int row_len;
    int64_t rows_cap; const int64_t *nrows;      // rows below min(rows_cap, *nrows); nrows NULL = rows_cap
    const uint8_t *mask; const int32_t *seg;     // either may be NULL: every cell counts
    const int32_t *start_plane, *end_plane;      // both or neither: whole-word units / every cell its own unit
    MlmSpec spec;                                // thresholds, generator key, ids; the specials by value
    int32_t *ids_out, *labels_out;               // [rows_cap * row_len] each, either may be NULL; ids_out may be `rows`
};
void launch_rows_mlm(const RowsMlmParams &p, hipStream_t s);

// RowsMlmPredictionsBatchDevice (additive; k_rows_mlm_cap in bf_kernels_mlm.hip): the same masking with at most max_pred > 0 predictions per row, gathered
struct RowsMlmCapParams {
    RowsMlmParams m;                             // as above; labels_out and ids_out may both be NULL when a gathered output is taken
    int max_pred;                                // P, 1 .. MLM_CAP_MAX_PRED; row_len <= MLM_CAP_MAX_LEN
    int32_t *pred_cell, *pred_label;             // [rows_cap * P] each: the kept cells in cell order and their original ids, then 0 / ignore_label; either may be NULL
    int32_t *pred_count;                         // [rows_cap]: kept cells of the row; may be NULL
};
void launch_rows_mlm_cap(const RowsMlmCapParams &p, hipStream_t s);

// RowsDenoiseBatchDevice (additive; bf_denoise.h has the lane code, k_rows_denoise in bf_kernels_denoise.hip): span corruption of rows that are already
// there, the encoder row and the decoder row compacted in one walk
struct RowsDenoiseParams {
    const int32_t *rows; int row_len;
    int64_t rows_cap; const int64_t *nrows;      // rows below min(rows_cap, *nrows); nrows NULL = rows_cap
    const uint8_t *mask; const int32_t *seg;     // either may be NULL: every cell counts
    DenoiseSpec spec;                            // thresholds, lengths, sentinels, generator key, ids; the specials by value
    int enc_len; int32_t *enc, *enc_cell;        // [rows_cap * enc_len] each, either may be NULL; enc_len counts only where one is taken
    int dec_len; int32_t *dec, *dec_cell;        // [rows_cap * dec_len] each, likewise
    int32_t *enc_count, *dec_count, *span_count; // [rows_cap] each, any may be NULL
    int *status;                                 // bit 0: a row lost a cell of an output the caller takes
};
void launch_rows_denoise(const RowsDenoiseParams &p, hipStream_t s);

// IdsToPackedRowsBatch (additive; bf_packed.h has the lane code, bf_kernels_packed.hip the kernels): several sequences per row, with a segment
// and a position plane.  Every workspace array has nseq + 1 entries (index nseq = the end of the chain) unless noted.
struct PackedParams {
    PackedSpec spec;
    const int32_t *ids; int64_t ids_len; const int64_t *id_off; int64_t nseq; int *status;
    int32_t *widths;             // [nseq] unit widths, scanned into W
    int64_t *W;                  // exclusive scan of the widths
    int32_t *jmp[2];             // next(s), squared round by round from one buffer into the other
    int32_t *mark;               // 1 = a row starts at this sequence
    int64_t *mark_off;           // exclusive scan of mark[0 .. nseq): rows in front of a sequence's row start; mark_off[nseq] = R
    int32_t *f;                  // the sequence every row starts at, f[R] = nseq
    int64_t rows_cap;            // no row r >= rows_cap of a plane is written, no entry past min(R, rows_cap) of row_first
    int32_t *rows, *seg, *pos;   // [rows_cap * row_len] each, any may be NULL
    int32_t *row_first;          // [rows_cap + 1], may be NULL
    int32_t *seq_row, *seq_col;  // [nseq] each, either may be NULL
    int64_t *nrows;              // [1]
};
void launch_packed_widths(const PackedParams &p, hipStream_t s);                // lane per sequence: widths, status bit 3
void launch_packed_next(const PackedParams &p, hipStream_t s);                  // lane per sequence: jmp[0] = next, mark = {0}
void launch_packed_double(const PackedParams &p, int round, hipStream_t s);     // one doubling round: reads jmp[round & 1], writes the other
void launch_packed_rows(const PackedParams &p, hipStream_t s);                  // behind the scan of the marks: f, row_first, seq_row, nrows, status bit 0
void launch_packed_cols(const PackedParams &p, hipStream_t s);                  // seq_col
void launch_packed_fill(const PackedParams &p, hipStream_t s);                  // the three planes
// IdsToPackedRowsPlanesBatch (additive): up to ROWS_MAX_PLANES int32 arrays parallel to the ids, gathered into planes with the layout of `rows` by
// k_packed_planes, behind the kernels of the base call.  A struct of its own: the kernels above keep their arguments where they are.
struct PackedPlanesParams {
    PackedParams pk;             // the call's packed stage as its kernels saw it: W, f and the row count are in the workspaces when the kernel runs
    int nplanes;
    const int32_t *src[ROWS_MAX_PLANES];         // parallel to the ids; read at id cells alone (NULL only where there is no id to read)
    int32_t fill[ROWS_MAX_PLANES];               // what a cell without an id gets
    int32_t *out[ROWS_MAX_PLANES];               // [rows_cap * row_len] each; NULL = not taken
};
void launch_packed_planes(const PackedPlanesParams &p, hipStream_t s);          // the planes taken; rows dropped from them (status bit 0)
// IdsToStreamRowsBatch (additive; bf_stream.h has the lane code, bf_kernels_stream.hip the kernels): the units laid end to end and cut into rows,
// with labels, a segment and a position plane.  Its workspaces are the first three of the packed stage: widths, block sums, W.
struct StreamParams {
    StreamSpec spec;
    const int32_t *ids; int64_t ids_len; const int64_t *id_off; int64_t nseq; int *status;
    int32_t *widths;             // [nseq] unit widths, scanned into W
    int64_t *W;                  // [nseq + 1] exclusive scan of the widths; W[nseq] = T
    int64_t rows_cap;            // no row r >= rows_cap of a row output is written
    int32_t *rows, *seg, *pos, *labels;          // [rows_cap * row_len] each, any may be NULL
    int32_t *row_first_seq, *row_first_pos;      // [rows_cap] each, either may be NULL
    int32_t *seq_row, *seq_col;  // [nseq] each, either may be NULL
    int64_t *nrows;              // [2] = {R, T}
};
void launch_stream_widths(const StreamParams &p, hipStream_t s);                // lane per sequence: widths, status bit 3
void launch_stream_seq(const StreamParams &p, hipStream_t s);                   // behind the scan: seq_row, seq_col, nrows, status bit 0
void launch_stream_fill(const StreamParams &p, int64_t rows_bound, hipStream_t s);      // the four planes and the row-first pair, tile by tile
// ByteToCharOffsetsBatchDevice / CharToByteOffsetsBatchDevice (additive; bf_charpos.h has the lane code, bf_kernels_charpos.hip the kernels): the
// index over 64-byte chunks of the text (masks, weights, their scan P) and the per-item conversion.  unit 0: `four` is NULL.
struct CharposParams {
    const uint8_t *text; int64_t total_bytes, nchunks;
    uint64_t *lead, *four;       // [nchunks] each: the bytes with a weight; the bytes >= 0xF0 (UTF-16 alone)
    int32_t *counts;             // [nchunks] weight of a chunk, scanned into P
    int64_t *P;                  // [nchunks + 1]
    const int64_t *doc_off; int64_t ndocs;
    const int64_t *item_off;     // [ndocs + 1], or NULL: item d belongs to document d
    int64_t items_cap;
    const int32_t *starts, *ends; int32_t *starts_out, *ends_out;      // either pair may be NULL
    int32_t *doc_units;          // [ndocs] U_d, may be NULL
    int dir, flags;              // CHARPOS_FWD / CHARPOS_INV; CHARPOS_ENDS_*
    int *status;
};
void launch_char_index(const CharposParams &p, hipStream_t s);                  // the pass over the text: masks and weights
void launch_char_docs(const CharposParams &p, hipStream_t s);                   // behind the scan: status bit 3 of a bad range, U_d
void launch_char_items(const CharposParams &p, int64_t items_bound, hipStream_t s);     // k_char_fwd / k_char_inv, a lane per item
void launch_compact(const CompactParams &p, hipStream_t s);
int scan_nblocks(int64_t ndocs);

} // namespace bfa
