/*
 * blingfiretokdll_amd.h -- C-ABI of the MI355X-native drop-in for BlingFire's
 * libblingfiretokdll (TextToIds hot path).
 *
 * The library is built as blingfire_amd/libblingfiretokdll.so and exports the SAME
 * unmangled extern "C" symbols the reference's wrappers bind by name
 * (reference: blingfiretools/blingfiretokdll/blingfiretokdll.h:23-104,
 *  blingfiretools/blingfiretokdll/blingfiretokdll.def:3-26,
 *  dist-pypi/blingfire/__init__.py:16-22,243-253, nuget/lib/BlingFireUtils.cs:23-35,195-215).
 *
 * All compute happens on the GPU (HIP, gfx950).  There is no CPU fallback: without a HIP
 * device LoadModel/SetModel print a diagnostic to stderr and return NULL.
 *
 * Plain pointers and sizes only; no C++/torch types.  Batch entry points (additive, not in
 * the reference) take either host buffers or device buffers + a hipStream_t passed as void*.
 */
#ifndef BLINGFIRETOKDLL_AMD_H
#define BLINGFIRETOKDLL_AMD_H

#include <stdint.h>
#ifndef __cplusplus
#include <stdbool.h>
#endif

/* The library is built with -fvisibility=hidden: only the entry points declared here (and the experiment knobs of
 * blingfire_amd/csrc/bf_internal.h) are exported. */
#if defined(__GNUC__)
#define BF_API __attribute__((visibility("default")))
#else
#define BF_API
#endif

#ifdef __cplusplus
extern "C" {
#endif

/* ---- reference entry points (same names, argument meaning and error behaviour) ---- */

/* reference tokdll:107-111: returns 18000 for v0.1.8-compatible behaviour */
BF_API int GetBlingFireTokVersion(void);

/* reference tokdll:1077-1094.  Returns an opaque handle or NULL.  (The reference throws a C++
 * exception through the C boundary for a nonexistent file; this returns NULL instead.) */
BF_API void *LoadModel(const char *pszLdbFileName);

/* reference tokdll:1056-1070.  The image is copied (the reference borrows it). */
BF_API void *SetModel(const unsigned char *pImgBytes, int ModelByteCount);

/* reference tokdll:1650-1662.  Returns 1, or 0 for a NULL handle. */
BF_API int FreeModel(void *ModelPtr);

/* reference tokdll:1619-1646.  Writes at most MaxIdsArrLength ids, leaves the rest of pIdsArr
 * untouched, returns the number written; 0 on any error (NULL model/text, n <= 0, n > 1e9,
 * invalid UTF-8 for non-byte models). */
BF_API int TextToIds(void *ModelPtr, const char *pInUtf8Str, int InUtf8StrByteCount,
              int32_t *pIdsArr, const int MaxIdsArrLength, const int UnkId);

/* reference tokdll:1320-1331 and 1541-1552: the two algorithm-specific spellings */
BF_API int TextToIds_wp(void *ModelPtr, const char *pInUtf8Str, int InUtf8StrByteCount,
                 int32_t *pIdsArr, const int MaxIdsArrLength, const int UnkId);
BF_API int TextToIds_sp(void *ModelPtr, const char *pInUtf8Str, int InUtf8StrByteCount,
                 int32_t *pIdsArr, const int MaxIdsArrLength, const int UnkId);

/* reference tokdll:1562-1609 (dispatch), 1108-1314 (_wp), 1349-1535 (_sp): ids plus, for every id, the byte offset of its first
 * character and the INCLUSIVE byte offset of the last byte of its last character in the caller's string (a BOM counts; the
 * dummy prefix has offset -1).  NULL pStartOffsets / pEndOffsets = ids only, exactly like the reference.  One deviation: for a
 * token made of the dummy prefix alone the reference adds the UTF-8 size of the byte BEFORE the caller's buffer (undefined);
 * this library reports end = -1. */
BF_API int TextToIdsWithOffsets(void *ModelPtr, const char *pInUtf8Str, int InUtf8StrByteCount, int32_t *pIdsArr,
                         int *pStartOffsets, int *pEndOffsets, const int MaxIdsArrLength, const int UnkId);
BF_API int TextToIdsWithOffsets_wp(void *ModelPtr, const char *pInUtf8Str, int InUtf8StrByteCount, int32_t *pIdsArr,
                            int *pStartOffsets, int *pEndOffsets, const int MaxIdsArrLength, const int UnkId);
BF_API int TextToIdsWithOffsets_sp(void *ModelPtr, const char *pInUtf8Str, int InUtf8StrByteCount, int32_t *pIdsArr,
                            int *pStartOffsets, int *pEndOffsets, const int MaxIdsArrLength, const int UnkId);

/* reference tokdll:610-614, 585-591, 569-575, 415-566: splits text into words with a lexer model (hModel == NULL: the built-in
 * wbd.bin, embedded like the reference embeds it).  Output = words joined by ' ' (inner spaces -> '_') + terminating 0; returns
 * the byte count needed (terminator included; copied only if it fits), 0 for empty input, -1 on error (invalid UTF-8, ...).
 * pStartOffsets / pEndOffsets (MaxOutUtf8StrByteCount entries each, may be NULL) receive the byte span of every word.
 * The tokenisation runs on the GPU; only the output string is assembled on the host. */
BF_API int TextToWords(const char *pInUtf8Str, int InUtf8StrByteCount, char *pOutUtf8Str, const int MaxOutUtf8StrByteCount);
BF_API int TextToWordsWithModel(const char *pInUtf8Str, int InUtf8StrByteCount, char *pOutUtf8Str, const int MaxOutUtf8StrByteCount, void *hModel);
BF_API int TextToWordsWithOffsets(const char *pInUtf8Str, int InUtf8StrByteCount, char *pOutUtf8Str, int *pStartOffsets, int *pEndOffsets,
                           const int MaxOutUtf8StrByteCount);
BF_API int TextToWordsWithOffsetsWithModel(const char *pInUtf8Str, int InUtf8StrByteCount, char *pOutUtf8Str, int *pStartOffsets,
                                    int *pEndOffsets, const int MaxOutUtf8StrByteCount, void *hModel);

/* additive: TextToWords for many documents at once.  The output string of document d -- exactly
 * what TextToWordsWithModel writes for it, without the terminating 0; nothing for a document it would reject -- is
 * text_out[text_offsets_out[d] .. text_offsets_out[d+1]).  ModelPtr NULL = the built-in wbd.bin.  Returns the total byte count
 * or BF_E_* (BF_E_CAPACITY: the offsets are valid and tell the size).  The Device form takes device pointers and a hipStream_t
 * and never writes past text_cap; with d_text_out == NULL it only computes the offsets.  Tokenisation AND string assembly
 * (a variable-length byte gather) run on the GPU. */
BF_API int64_t TextToWordsBatch(void *ModelPtr, const char *text, const int64_t *doc_offsets, int64_t ndocs, char *text_out, int64_t text_cap,
                         int64_t *text_offsets_out);
BF_API int TextToWordsBatchDevice(void *ModelPtr, const char *d_text, const int64_t *d_doc_offsets, int64_t ndocs, int64_t total_bytes,
                           char *d_text_out, int64_t text_cap, int64_t *d_text_offsets_out, void *stream);
/* the same for TextToSentences (ModelPtr NULL = the built-in sbd.bin): per document the string TextToSentencesWithModel writes */
BF_API int64_t TextToSentencesBatch(void *ModelPtr, const char *text, const int64_t *doc_offsets, int64_t ndocs, char *text_out, int64_t text_cap,
                             int64_t *text_offsets_out);
BF_API int TextToSentencesBatchDevice(void *ModelPtr, const char *d_text, const int64_t *d_doc_offsets, int64_t ndocs, int64_t total_bytes,
                               char *d_text_out, int64_t text_cap, int64_t *d_text_offsets_out, void *stream);

/* reference tokdll:163-402 (blingfiretokdll.def: TextToSentences, TextToSentencesWithModel, TextToSentencesWithOffsets,
 * TextToSentencesWithOffsetsWithModel): sentence breaking with the model behind hModel (a LoadModel handle of a [wbd]-type
 * model such as sbd.bin; NULL = the built-in sbd.bin, embedded like the reference embeds it).  Output = sentences joined by
 * '\n' (a '\n' inside a sentence -> ' ', leading white space dropped) + terminating 0; same return convention and offset
 * arrays as TextToWords.  The sentence boundaries come from the GPU lexer; only the output string is assembled on the host. */
BF_API int TextToSentences(const char *pInUtf8Str, int InUtf8StrByteCount, char *pOutUtf8Str, const int MaxOutUtf8StrByteCount);
BF_API int TextToSentencesWithModel(const char *pInUtf8Str, int InUtf8StrByteCount, char *pOutUtf8Str, const int MaxOutUtf8StrByteCount, void *hModel);
BF_API int TextToSentencesWithOffsets(const char *pInUtf8Str, int InUtf8StrByteCount, char *pOutUtf8Str, int *pStartOffsets, int *pEndOffsets,
                               const int MaxOutUtf8StrByteCount);
BF_API int TextToSentencesWithOffsetsWithModel(const char *pInUtf8Str, int InUtf8StrByteCount, char *pOutUtf8Str, int *pStartOffsets,
                                        int *pEndOffsets, const int MaxOutUtf8StrByteCount, void *hModel);

/* reference tokdll:629-679 (blingfiretokdll.def: NormalizeSpaces; model-free): every run of white space -> one uSpace (default
 * U+2581 in the reference's header), leading white space dropped, one trailing uSpace trimmed; returns the output byte count
 * (0-terminated when there is room), -1 for empty / invalid UTF-8 input or when the output does not fit.  Runs as a batch of
 * one on the GPU; NormalizeSpacesBatch (additive) does many documents, output layout like TextToWordsBatch (a document the
 * single call rejects yields nothing). */
BF_API int NormalizeSpaces(const char *pInUtf8Str, int InUtf8StrByteCount, char *pOutUtf8Str, const int MaxOutUtf8StrByteCount, const int uSpace);
BF_API int64_t NormalizeSpacesBatch(const char *text, const int64_t *doc_offsets, int64_t ndocs, char *text_out, int64_t text_cap,
                             int64_t *text_offsets_out, int uSpace);

/* reference tokdll:773-806 (blingfiretokdll.def: TextToHashes; model-free): fasttext-style hashes of the space-separated tokens
 * of an already tokenised string, followed by the word n-gram hashes modulo bucketSize; returns the number of hashes,
 * InUtf8StrByteCount * wordNgrams ("requested size") when MaxHashArrLength is too small, -1 on error.  Deviation: wordNgrams <= 0
 * is refused (-1); the reference would write past the array.  TextToHashesBatch (additive): document d's hashes =
 * hashes_out[hash_offsets_out[d] .. hash_offsets_out[d+1]), (spaces + 1) * wordNgrams of them. */
BF_API int TextToHashes(const char *pInUtf8Str, int InUtf8StrByteCount, int32_t *pHashArr, const int MaxHashArrLength, int wordNgrams, int bucketSize);
BF_API int64_t TextToHashesBatch(const char *text, const int64_t *doc_offsets, int64_t ndocs, int32_t *hashes_out, int64_t hashes_cap,
                          int64_t *hash_offsets_out, int wordNgrams, int bucketSize);

/* reference tokdll:1689-1745 (blingfiretokdll.def: IdsToText): text of an id sequence.  ModelPtr = a LoadModel handle of a
 * model with an [i2w] section (a *.i2w file, or a .bin that carries one).  Ids outside the model's regular range are left
 * out when SkipSpecialTokens is set; a leading space is not written; returns the byte count needed including the
 * terminating 0 (written when it fits), 0 on error (no [i2w], unknown id, ...).  Runs as a batch of one on the GPU. */
BF_API int IdsToText(void *ModelPtr, const int32_t *pIdsArr, const int IdsCount, char *pOutUtf8Str, const int MaxOutUtf8StrByteCount,
              bool SkipSpecialTokens);

/* additive: many sequences at once.  ids of sequence d = ids[id_offsets[d] .. id_offsets[d+1]); its text (no terminator) =
 * text_out[text_offsets_out[d] .. text_offsets_out[d+1]), exactly the bytes IdsToText produces for it; a sequence with an
 * unknown id yields no text.  Returns the total byte count or BF_E_* (BF_E_CAPACITY if text_cap is too small: the offsets
 * are valid then and tell the size).  The Device form takes device pointers and a hipStream_t; with d_text_out == NULL it
 * only computes the offsets (size query). */
BF_API int64_t IdsToTextBatch(void *ModelPtr, const int32_t *ids, const int64_t *id_offsets, int64_t nseq, char *text_out, int64_t text_cap,
                       int64_t *text_offsets_out, int skip_special);
BF_API int IdsToTextBatchDevice(void *ModelPtr, const int32_t *d_ids, const int64_t *d_id_offsets, int64_t nseq, char *d_text_out,
                         int64_t text_cap, int64_t *d_text_offsets_out, int skip_special, void *stream);

/* additive (no counterpart in the reference; this comment is the specification): fixed-shape model inputs from ragged ids, e.g. the
 * d_ids_out / d_id_offsets_out of TextToIdsBatchDevice as they are.  Sequence q = ids[id_offsets[q] .. id_offsets[q+1]), n ids.  With
 * body = row_len - (cls_id >= 0) - (sep_id >= 0) and step = body - stride, it yields 1 row when n <= body (an empty sequence too), else
 * 1 + ceil((n - body) / step) rows, at most max_rows_per_seq of them when that is > 0 (1 = truncate, 0 = all windows).  Row w of a sequence
 * holds its ids [w * step, min(n, w * step + body)):  [cls_id] ids... [sep_id] pad_id...  (flags bit 0: the padding comes first); the mask
 * is 1 over the ids and the specials, 0 over the padding.  cls_id / sep_id < 0 = no such special.  Rows come in sequence order, windows
 * in order.  BF_E_ARG unless 1 <= row_len <= 1 << 20, body >= 1, 0 <= stride < body, max_rows_per_seq >= 0 and no other flag bit is set.
 * ModelPtr: any live handle (it lends its device, workspaces and status word; the model is not consulted); NULL = BF_E_ARG.
 * Device form: enqueues on `stream` (a hipStream_t), does not synchronise, returns 0 or BF_E_*.  ids_len = the elements of d_ids that may
 * be read (the capacity of the tokenizer's id array will do: the exact total is on the device only); a sequence whose range is not inside
 * [0, ids_len] or whose offsets decrease counts as empty and sets BfLastStatus bit 3 -- chaining behind a tokenizer call that overflowed
 * its ids_cap is safe.  d_row_offsets_out[nseq+1] is always complete: the rows of sequence q are [off[q], off[q+1]).  d_rows_out and
 * d_mask_out ([rows_cap * row_len] each), d_row_seq_out (the sequence of every row) and d_row_first_out (the index within its sequence of
 * the row's first id; [rows_cap] each) may each be NULL; all four NULL = a size query.  No row r >= rows_cap of any output is written;
 * rows dropped that way, and a row count or a d_row_first_out value of one sequence beyond INT32_MAX (they saturate), set BfLastStatus bit 0 (the call clears the
 * status word first, like every batch call: what an earlier call on the handle reported is gone).  After
 * BfReserve(h, max_docs >= nseq, ...) the call allocates nothing.  16-byte aligned d_rows_out, 4-byte aligned d_mask_out and
 * row_len % 4 == 0 take the wide stores.  Host form: returns the row total, or BF_E_CAPACITY with complete offsets and nothing else written; with all four
 * outputs NULL it is a size query that returns the total whatever rows_cap is.  id_offsets[0] < 0 = BF_E_ARG. */
BF_API int IdsToRowsBatchDevice(void *ModelPtr, const int32_t *d_ids, int64_t ids_len, const int64_t *d_id_offsets, int64_t nseq,
                         int row_len, int cls_id, int sep_id, int pad_id, int stride, int max_rows_per_seq, int flags,
                         int32_t *d_rows_out, uint8_t *d_mask_out, int32_t *d_row_seq_out, int32_t *d_row_first_out,
                         int64_t rows_cap, int64_t *d_row_offsets_out, void *stream);
BF_API int64_t IdsToRowsBatch(void *ModelPtr, const int32_t *ids, const int64_t *id_offsets, int64_t nseq,
                       int row_len, int cls_id, int sep_id, int pad_id, int stride, int max_rows_per_seq, int flags,
                       int32_t *rows_out, uint8_t *mask_out, int32_t *row_seq_out, int32_t *row_first_out,
                       int64_t rows_cap, int64_t *row_offsets_out);

/* additive (no counterpart in the reference; this comment is the specification): fixed-shape model inputs from PAIRS of ragged id sequences,
 * [cls] A [sep] B [sep] with token type ids -- cross-encoder / NLI inputs, and extractive-QA windows whose question is repeated in every row.
 * Pair q of nseq is A = ids_a[off_a[q] .. off_a[q+1]) (na ids) and B = ids_b[off_b[q] .. off_b[q+1]) (nb ids), e.g. the d_ids_out /
 * d_id_offsets_out of two TextToIdsBatchDevice calls as they are; ids_a and ids_b may be the same array.
 * Specials: cls_id < 0 = no leading special; sep_id < 0 = no separators at all; with sep_id >= 0 one separator stands between A and B (two
 * with flags bit 1, the RoBERTa form) and one behind B.  S = the number of specials, T = row_len - S = the room for ids.  A row is
 *     [cls_id] A' [sep_id]([sep_id]) B' [sep_id] pad_id...                   (flags bit 0: the padding comes first)
 * the mask is 1 over everything but the padding; the type byte is 0 over cls, A' and the middle separator(s), 1 over B' and the trailing
 * separator, 0 over the padding.
 * mode 0, window the second sequence: ka = min(na, max_a) and A' = the first ka ids of A, in every row of the pair.  The pair's own geometry
 * is body_b = T - ka and step = body_b - stride: it yields 1 row when nb <= body_b (nb = 0 too), else 1 + ceil((nb - body_b) / step) rows, at
 * most max_rows_per_pair of them when that is > 0 (1 = truncate B, 0 = all windows).  Row w of the pair holds B[w * step .. min(nb, w * step +
 * body_b)).  BF_E_ARG unless 0 <= max_a <= T - 1, 0 <= stride < T - max_a and max_rows_per_pair >= 0 (every pair then has body_b >= 1 and
 * step >= 1: no pair can fail on its own).
 * mode 1, longest first, one row per pair: ids are dropped from the end of the longer sequence, one at a time, until ka + kb <= T; on a tie the
 * id is dropped from B.  (In closed form ka = min(na, max(ceil(T / 2), T - nb)), kb = min(nb, T - ka); truncating both inputs to T ids first
 * does not change the result.)  A' / B' = the first ka / kb ids.  BF_E_ARG unless max_a == 0, stride == 0 and max_rows_per_pair == 1.
 * BF_E_ARG also for row_len outside 1 .. 1 << 20, T < 1, a mode other than 0 and 1, another flag bit, flags bit 1 with sep_id < 0 and a NULL
 * ModelPtr (any live handle: it lends its device, workspaces and status word; the model is not consulted).  Rows come in pair order, windows
 * in order.
 * Device form: enqueues on `stream` (a hipStream_t), does not synchronise, returns 0 or BF_E_*.  ids_a_len / ids_b_len = the elements of
 * d_ids_a / d_ids_b that may be read (capacities, exactly as ids_len of IdsToRowsBatchDevice); a range that is not inside [0, len] or whose
 * offsets decrease makes that side of its pair empty and sets BfLastStatus bit 3.  d_row_offsets_out[nseq+1] is always complete: the rows of
 * pair q are [off[q], off[q+1]).  d_rows_out (int32), d_mask_out and d_type_out (uint8; [rows_cap * row_len] each), d_row_seq_out (the pair of
 * every row) and d_row_first_b_out (the index within B of the row's first B id, w * step, saturating at INT32_MAX; [rows_cap] each) may each
 * be NULL; all five NULL = a size query.  No row r >= rows_cap of any output is written; rows dropped that way, and a saturated row count or
 * first-id index, set BfLastStatus bit 0 (the call clears the status word first).  After BfReserve(h, max_docs >= nseq, ...) the call allocates
 * nothing.  Every pointer needs only the natural alignment of its type; 16-byte aligned d_rows_out, 4-byte aligned d_mask_out and d_type_out
 * and row_len % 4 == 0 take the wide stores.
 * Host form: returns the row total, or BF_E_CAPACITY with complete offsets and nothing else written; with all five outputs NULL it is a size
 * query that returns the total whatever rows_cap is.  It reads each side from its first offset to its largest one; off_a[0] < 0 or
 * off_b[0] < 0 = BF_E_ARG. */
BF_API int IdsToPairRowsBatchDevice(void *ModelPtr, const int32_t *d_ids_a, int64_t ids_a_len, const int64_t *d_off_a,
                             const int32_t *d_ids_b, int64_t ids_b_len, const int64_t *d_off_b, int64_t nseq,
                             int row_len, int cls_id, int sep_id, int pad_id, int mode, int max_a, int stride, int max_rows_per_pair, int flags,
                             int32_t *d_rows_out, uint8_t *d_mask_out, uint8_t *d_type_out, int32_t *d_row_seq_out, int32_t *d_row_first_b_out,
                             int64_t rows_cap, int64_t *d_row_offsets_out, void *stream);
BF_API int64_t IdsToPairRowsBatch(void *ModelPtr, const int32_t *ids_a, const int64_t *off_a, const int32_t *ids_b, const int64_t *off_b, int64_t nseq,
                           int row_len, int cls_id, int sep_id, int pad_id, int mode, int max_a, int stride, int max_rows_per_pair, int flags,
                           int32_t *rows_out, uint8_t *mask_out, uint8_t *type_out, int32_t *row_seq_out, int32_t *row_first_b_out,
                           int64_t rows_cap, int64_t *row_offsets_out);

/* additive (no counterpart in the reference; this comment is the specification): COMPANION PLANES for IdsToRowsBatch / IdsToPairRowsBatch -- up
 * to BF_ROWS_MAX_PLANES int32 arrays that run parallel to the ids (the d_starts_out / d_ends_out of TextToIdsWithOffsetsBatchDevice as they
 * are, per-token labels, word indices, ...) are gathered into int32 planes of [rows_cap * row_len] cells with the layout of d_rows_out, in the
 * same call.  Element i of a source belongs to d_ids[i].  Plane k of nplanes: a cell that holds id number i of its sequence q gets
 * src[k][off[q] + i]; a cell that holds cls_id, a separator or padding gets fill[k].
 * IdsToRowsPlanesBatchDevice / IdsToRowsPlanesBatch take every argument of IdsToRowsBatchDevice / IdsToRowsBatch, with the same meaning, checks,
 * status bits and capacity rules, and behind d_row_offsets_out: nplanes, d_src, fill, d_planes_out -- three HOST arrays of nplanes entries whose
 * values travel to the kernel by value (d_src[k] and d_planes_out[k] are device pointers in the Device form, host pointers in the host form).
 * d_src[k] is read for at most ids_len elements, and only at cells that hold an id.  d_planes_out[k] may be NULL: that plane is skipped.
 * IdsToPairRowsPlanesBatchDevice / IdsToPairRowsPlanesBatch are the same over IdsToPairRowsBatchDevice / IdsToPairRowsBatch, with d_src_a (parallel
 * to d_ids_a) and d_src_b (parallel to d_ids_b).  Either array pointer, or any entry of one, may be NULL: the cells of that side then take fill[k]
 * -- the extractive-QA form is offsets over the context (B) alone and the fill over the question.
 * BF_E_ARG for nplanes outside 0 .. BF_ROWS_MAX_PLANES, a NULL fill or d_planes_out with nplanes > 0 and, in the rows form, a NULL d_src or
 * d_src[k] with ids_len > 0 (host form: with any id to read); and for whatever the base call refuses.
 * The calls are supersets of the base calls: rows, mask, type, row_seq, row_first and the row offsets are byte for byte what the base call
 * writes for the same arguments; with nplanes = 0 the call is the base call; a size query is every output and every plane NULL.  No row
 * r >= rows_cap of a plane is written; a sequence read as empty (BfLastStatus bit 3) has no id cells; rows dropped from a plane the caller takes
 * set BfLastStatus bit 0.  After BfReserve(h, max_docs >= nseq, ...) the Device forms allocate nothing.  Every pointer needs only the natural
 * alignment of its type: with row_len % 4 == 0 and every taken plane aligned to 16 bytes a lane makes one 16-byte store per plane, otherwise
 * it writes one cell; the sources are read element by element, because a sequence starts anywhere.
 * Host forms: each source is staged beside the ids (read, like them, from the side's first offset to its largest one); BF_E_CAPACITY with
 * complete offsets and nothing else written, exactly as the base calls.  Packed rows have companion planes of their own: IdsToPackedRowsPlanesBatch below. */
#define BF_ROWS_MAX_PLANES 4
BF_API int IdsToRowsPlanesBatchDevice(void *ModelPtr, const int32_t *d_ids, int64_t ids_len, const int64_t *d_id_offsets, int64_t nseq,
                               int row_len, int cls_id, int sep_id, int pad_id, int stride, int max_rows_per_seq, int flags,
                               int32_t *d_rows_out, uint8_t *d_mask_out, int32_t *d_row_seq_out, int32_t *d_row_first_out,
                               int64_t rows_cap, int64_t *d_row_offsets_out,
                               int nplanes, const int32_t *const *d_src, const int32_t *fill, int32_t *const *d_planes_out, void *stream);
BF_API int64_t IdsToRowsPlanesBatch(void *ModelPtr, const int32_t *ids, const int64_t *id_offsets, int64_t nseq,
                             int row_len, int cls_id, int sep_id, int pad_id, int stride, int max_rows_per_seq, int flags,
                             int32_t *rows_out, uint8_t *mask_out, int32_t *row_seq_out, int32_t *row_first_out,
                             int64_t rows_cap, int64_t *row_offsets_out,
                             int nplanes, const int32_t *const *src, const int32_t *fill, int32_t *const *planes_out);
BF_API int IdsToPairRowsPlanesBatchDevice(void *ModelPtr, const int32_t *d_ids_a, int64_t ids_a_len, const int64_t *d_off_a,
                                   const int32_t *d_ids_b, int64_t ids_b_len, const int64_t *d_off_b, int64_t nseq,
                                   int row_len, int cls_id, int sep_id, int pad_id, int mode, int max_a, int stride, int max_rows_per_pair, int flags,
                                   int32_t *d_rows_out, uint8_t *d_mask_out, uint8_t *d_type_out, int32_t *d_row_seq_out, int32_t *d_row_first_b_out,
                                   int64_t rows_cap, int64_t *d_row_offsets_out,
                                   int nplanes, const int32_t *const *d_src_a, const int32_t *const *d_src_b, const int32_t *fill,
                                   int32_t *const *d_planes_out, void *stream);
BF_API int64_t IdsToPairRowsPlanesBatch(void *ModelPtr, const int32_t *ids_a, const int64_t *off_a, const int32_t *ids_b, const int64_t *off_b, int64_t nseq,
                                 int row_len, int cls_id, int sep_id, int pad_id, int mode, int max_a, int stride, int max_rows_per_pair, int flags,
                                 int32_t *rows_out, uint8_t *mask_out, uint8_t *type_out, int32_t *row_seq_out, int32_t *row_first_b_out,
                                 int64_t rows_cap, int64_t *row_offsets_out,
                                 int nplanes, const int32_t *const *src_a, const int32_t *const *src_b, const int32_t *fill, int32_t *const *planes_out);

/* additive (no counterpart in the reference; this comment is the specification): SPAN CELLS -- an item's byte span, e.g. an answer inside a
 * context, as token cells of each of its rows.  Device only: it reads a start plane and an end plane that are already on the device
 * ([rows_cap * row_len] int32 each, e.g. two companion planes of the calls above over the tokenizer's starts and ends with fill -1), whatever
 * call laid the rows out: rows and pair rows alike.
 * Rows r < min(rows_cap, *d_nrows) are processed (d_nrows NULL = rows_cap rows; d_row_offsets_out + nseq of the row call before is the
 * intended d_nrows: nothing is read back); no entry at or past that bound of either output is written.  Row r belongs to item
 * q = d_row_seq ? d_row_seq[r] : r; a q outside [0, nseq) gives none_cell twice and sets BfLastStatus bit 3.
 * With a = d_span_first[q] and z = d_span_last[q] -- byte offsets in the coordinates of the planes, the last byte INCLUSIVE like the
 * tokenizer's ends -- S and E the row's cells of the two planes and C = { j : S[j] >= 0 }:
 *     a < 0, or z < a, or no j in C with S[j] <= a, or no j in C with E[j] >= z:   start_cell = end_cell = none_cell
 *     otherwise:   start_cell = max { j in C : S[j] <= a },   end_cell = min { j in C : E[j] >= z }
 * The definition assumes no ordering of the planes and neither does the kernel.  For offsets that rise along the row it is what the usual QA
 * preprocessing computes: the last token that starts at or before the answer and the first token that ends at or behind it.  With none_cell =
 * the cell of cls_id, an answer that is not fully inside the window gets the [CLS] cell (a window that begins behind a, or ends in front of z,
 * lacks one of the two candidates).  A token whose start is negative -- the dummy prefix of a SentencePiece model, the fill over a question --
 * is never an answer cell.
 * BF_E_ARG for row_len outside 1 .. 1 << 20, a negative rows_cap or nseq, a NULL plane, span array or output with rows_cap > 0, and a NULL
 * ModelPtr (any live handle, as for the row calls).  The call clears the status word first, like every batch call, enqueues on `stream`, does
 * not synchronise, allocates nothing and returns 0 or BF_E_*.  A wave shares a row (a power-of-two slice of a wave when row_len <= 32). */
BF_API int RowsSpanCellsBatchDevice(void *ModelPtr, const int32_t *d_start_plane, const int32_t *d_end_plane, int row_len,
                             int64_t rows_cap, const int64_t *d_nrows, const int32_t *d_row_seq, int64_t nseq,
                             const int32_t *d_span_first, const int32_t *d_span_last, int none_cell,
                             int32_t *d_start_cell_out, int32_t *d_end_cell_out, void *stream);

/* additive (no counterpart in the reference; this comment is the specification): MLM MASKING -- the masked input ids and the labels of
 * masked-language-model pretraining, token by token or whole words.  Device only: it reads rows that are already on the device
 * ([rows_cap * row_len] int32), whatever call laid them out: rows, pair rows and packed rows alike.
 * Rows r < min(rows_cap, *d_nrows) are processed (d_nrows NULL = rows_cap rows; d_row_offsets_out + nseq of a row call or d_nrows_out of the
 * packed call is the intended d_nrows: nothing is read back); nothing at or past that bound of either output is written.  c = r * row_len + j
 * is cell j of row r.
 * The draw.  W(r, j) = Philox4x32-10(counter = {lo32(r), hi32(r), j, epoch}, key = {lo32(seed), hi32(seed)}), four 32-bit words; r is the
 * row's index in the planes as an int64.  (Multipliers 0xD2511F53 and 0xCD9E8D57, key increments 0x9E3779B9 and 0xBB67AE85, ten rounds, a round
 * maps c to {hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)}, the key is bumped after every round.)  What a cell gets depends
 * on (seed, r, j, epoch) and the row's own contents alone: not on the grid, the number of rows or the order of calls.
 * Eligible cell.  d_mask == NULL or d_mask[c] != 0; and d_seg == NULL or d_seg[c] != 0 (the segment plane of the packed call: 0 = padding);
 * and d_rows[c] is none of special_ids[0 .. nspecial) -- a HOST array of at most BF_MLM_MAX_SPECIAL ids whose values travel to the kernel by
 * value (cls_id, sep_id, pad_id, ...).
 * Units.  Without offset planes (d_start_plane and d_end_plane both NULL) every cell is its own unit: h(j) = j.  With both planes
 * ([rows_cap * row_len] int32 each, e.g. two companion planes over the tokenizer's starts and ends with fill -1; S and E the row's cells), cell
 * j >= 1 CONTINUES cell j - 1 when both cells are eligible, S[j-1] >= 0 and S[j] >= 0, and S[j] - 1 == E[j-1]: ends are inclusive like the
 * tokenizer's, so this is byte adjacency -- `play` `##ing` is one unit, two tokens with white space between them are two.  h(j) = the largest
 * j' <= j that does not continue.  This is whole-word masking for WordPiece models; for models whose tokens carry their white space (the
 * SentencePiece family, byte-level BPE) the definition holds as written but its units need not coincide with words.
 * Thresholds, computed on the host in double: Ts = (uint64) floor(select_prob * 4294967296.0), Tm and Tr the same of mask_prob and
 * random_prob.  All comparisons below are in 64 bits, so a probability of 1 means always.
 * Decision for an eligible cell j: it is selected iff W(r, h(j))[0] < Ts -- the unit's head decides, a unit is selected whole.  If selected,
 * with w = W(r, j), the cell's OWN draw (the pieces of a word take their own action, as the usual whole-word collator has it):
 *     labels = d_rows[c];   w[1] < Tm: ids = mask_id;   else w[1] < Tm + Tr: ids = rand_lo + (int32)(((uint64)w[2] * (uint64)(rand_hi - rand_lo)) >> 32);
 *     else ids = d_rows[c]
 * A cell that is not selected, and every cell that is not eligible: ids = d_rows[c], labels = ignore_label.
 * Outputs.  d_ids_out and d_labels_out are [rows_cap * row_len] int32; either may be NULL, not both.  d_ids_out == d_rows (in place) is
 * allowed: a lane reads only its own cell of d_rows before it writes it, what it needs of the neighbour comes from the planes.
 * BF_E_ARG for row_len outside 1 .. 1 << 20, a negative rows_cap, a NULL d_rows or both outputs NULL with rows_cap > 0, one offset plane
 * without the other, nspecial outside 0 .. BF_MLM_MAX_SPECIAL, a NULL special_ids with nspecial > 0, a probability outside [0, 1] (a NaN
 * is), mask_prob + random_prob > 1.0, Tr > 0 without 0 <= rand_lo < rand_hi, and a NULL ModelPtr (any live handle, as for the row calls).
 * The call clears the status word first, like every batch call, and sets no bit of it; it enqueues on `stream`, does not synchronise and
 * returns 0 or BF_E_*.  It has no workspace: it allocates nothing, with and without BfReserve.  Every pointer needs only the natural
 * alignment of its type.  A wave shares a row (a power-of-two slice of a wave when row_len <= 32) and walks it in chunks of as many cells.
 * Not here: a host-buffer form.  (Span corruption, the T5 objective: RowsDenoiseBatchDevice below.  A cap on the predictions of a row, with the kept cells gathered:
 * RowsMlmPredictionsBatchDevice below.  Offset planes of packed rows: IdsToPackedRowsPlanesBatchDevice below, which also says when a unit can span
 * two sequences of a packed row.) */
#define BF_MLM_MAX_SPECIAL 8
BF_API int RowsMlmMaskBatchDevice(void *ModelPtr, const int32_t *d_rows, int row_len, int64_t rows_cap, const int64_t *d_nrows,
                           const uint8_t *d_mask, const int32_t *d_seg, const int32_t *d_start_plane, const int32_t *d_end_plane,
                           int nspecial, const int32_t *special_ids, double select_prob, double mask_prob, double random_prob,
                           int mask_id, int rand_lo, int rand_hi, int ignore_label, uint64_t seed, uint32_t epoch,
                           int32_t *d_ids_out, int32_t *d_labels_out, void *stream);

/* additive (no counterpart in the reference; this comment is the specification): MLM PREDICTIONS -- RowsMlmMaskBatchDevice with a cap of
 * max_pred predictions per row (max_predictions_per_seq of the BERT data pipeline) and the predicted cells gathered, so that the output
 * projection of a masked language model runs on [rows, P] positions of a fixed shape instead of [rows, row_len].
 * Every argument from d_rows to d_labels_out is RowsMlmMaskBatchDevice's, and so are, word for word: the rows processed
 * (r < min(rows_cap, *d_nrows)), the draw W(r, j), eligibility, the units h(j), the thresholds, selection (W(r, h)[0] < Ts, a unit is selected
 * whole) and the action of a cell from its own w[1], w[2].  New:
 * Key.  A selected unit with head h has the 64-bit key K(h) = ((uint64)W(r, h)[3] << 32) | (uint32)h -- word 3 of the draw, which the base
 * call does not use.  Keys of distinct units of a row differ because their heads differ.
 * Count.  f(h) = the number of selected cells j' of the row with K(h(j')) <= K(h): the cells of the unit itself and of every selected unit
 * with a smaller key.
 * Cap.  max_pred = 0: every selected unit is kept.  max_pred = P > 0: a selected unit is kept iff f(h) <= P.  The kept units are therefore a
 * prefix of the selected units in key order, cut in front of the first unit that no longer fits: a later, smaller unit is NOT taken after
 * the cut.  A unit of more than P cells is never kept; where such a unit has the row's smallest key, the row has no predictions.  The rule
 * depends on (seed, r, epoch) and the row alone, prefers no position of the row (the keys are draws), keeps whole words whole and needs no
 * sequential walk.
 * Cells.  A cell of a kept unit gets what a selected cell gets in the base call: labels = d_rows[c], ids by its own draw.  Every other cell
 * -- a selected cell that the cap dropped included -- gets ids = d_rows[c], labels = ignore_label.  n_r = the kept cells of row r; n_r <= P.
 * Where P >= the selected cells of every row, ids and labels are byte for byte the base call's.
 * Gathered outputs (P > 0 only).  With j_0 < ... < j_{n_r - 1} the kept cells of row r in cell order:
 *     d_pred_cell_out[r * P + k] = j_k;   d_pred_label_out[r * P + k] = the ORIGINAL d_rows[r * row_len + j_k] (also when the call runs in place);
 *     for n_r <= k < P the two entries are 0 and ignore_label (a weight plane is label != ignore_label);   d_pred_count_out[r] = n_r
 * Their shapes are [rows_cap * P], [rows_cap * P] and [rows_cap].  Nothing at or past the row bound is written in any of the five outputs.
 * Any of the five outputs may be NULL; all five NULL with rows_cap > 0 is BF_E_ARG.  d_ids_out == d_rows (in place) stays allowed; the
 * gathered outputs must not overlap d_rows.
 * BF_E_ARG for whatever the base call refuses; max_pred < 0 or max_pred > 1 << 20; max_pred > 0 with row_len > BF_MLM_CAP_MAX_LEN (the
 * call has no workspace: the keys of a row stay on the chip, 8 bytes per cell, and beyond that length they do not fit a wave's share of
 * LDS); max_pred == 0 with a gathered output that is not NULL (there is no width to lay it out in).
 * With max_pred == 0 the call IS the base call: the same kernel launch and byte for byte the same outputs.
 * As there: the call clears the status word first and sets no bit of it; it enqueues on `stream`, does not synchronise and returns 0 or
 * BF_E_*; it has no workspace and allocates nothing, with and without BfReserve; every pointer needs only the natural alignment of its type.
 * Not here: BERT's skip-and-continue (a later unit that still fits is taken there: a sequential walk); span corruption is
 * RowsDenoiseBatchDevice below. */
#define BF_MLM_CAP_MAX_LEN 4096
BF_API int RowsMlmPredictionsBatchDevice(void *ModelPtr, const int32_t *d_rows, int row_len, int64_t rows_cap, const int64_t *d_nrows,
                           const uint8_t *d_mask, const int32_t *d_seg, const int32_t *d_start_plane, const int32_t *d_end_plane,
                           int nspecial, const int32_t *special_ids, double select_prob, double mask_prob, double random_prob,
                           int mask_id, int rand_lo, int rand_hi, int ignore_label, uint64_t seed, uint32_t epoch,
                           int32_t *d_ids_out, int32_t *d_labels_out, int max_pred, int32_t *d_pred_cell_out, int32_t *d_pred_label_out,
                           int32_t *d_pred_count_out, void *stream);

/* additive (no counterpart in the reference; this comment is the specification): SPAN CORRUPTION -- the encoder inputs and the decoder targets
 * of the denoising objective of the T5 / mT5 / UL2 family.  Noise spans collapse to one sentinel id in the encoder row and are listed behind
 * their sentinels in the decoder row, so every row is compacted twice, at different rates.  Device only: it reads rows that are already on the
 * device ([rows_cap * row_len] int32), whatever call laid them out: rows, packed rows and stream rows alike.
 * Rows processed.  Rows r < min(rows_cap, *d_nrows) are processed (d_nrows NULL = rows_cap rows; d_row_offsets_out + nseq of a row call or
 * d_nrows_out of the packed or the stream call is the intended d_nrows: nothing is read back); nothing at or past that bound of any output is
 * written.  c = r * row_len + j is cell j of row r.
 * The draw.  W(r, j) is RowsMlmMaskBatchDevice's, word for word: Philox4x32-10(counter = {lo32(r), hi32(r), j, epoch}, key = {lo32(seed),
 * hi32(seed)}), four 32-bit words.
 * Present and eligible.  A cell is PRESENT iff (d_mask == NULL or d_mask[c] != 0) and (d_seg == NULL or d_seg[c] != 0).  It is ELIGIBLE iff it is
 * present and d_rows[c] is none of special_ids[0 .. nspecial) -- a HOST array of at most BF_MLM_MAX_SPECIAL ids (eos_id, pad_id, ...).
 * Starts and lengths.  Ts = (uint64) floor(start_prob * 4294967296.0), computed on the host in double and compared in 64 bits, so a
 * probability of 1 means always.  An eligible cell h STARTS iff W(r, h)[0] < Ts, and then
 *     len(h) = len_lo + (int)(((uint64)W(r, h)[1] * (uint64)(len_hi - len_lo + 1)) >> 32)
 * -- uniform on [len_lo, len_hi], one Philox evaluation per eligible cell.
 * Raw noise.  Cell j is raw noise iff it is eligible and there is an h <= j such that every cell of [h, j] is eligible, h starts and
 * h + len(h) > j.  An ineligible cell (a special, padding, a cell outside the mask) therefore ends every span in front of it: no span
 * crosses the [SEP] or </s> between two sequences of a packed or stream row, and a span that reaches past the row's end is cut there.
 * Runs and the sentinel cap.  A run is a maximal stretch of consecutive raw-noise cells; overlapping and abutting spans are one run.  Runs
 * are numbered k = 0, 1, ... in cell order.  A run with k >= max_sentinels is not noise: its cells are copied like any other.  NOISE cells are
 * the cells of the runs k < max_sentinels; a run's BEGIN is its first cell; run k has the sentinel id sentinel_first + k * sentinel_step (T5:
 * sentinel_first 32099, sentinel_step -1, max_sentinels 100).  keep(<j), noise(<j), begins(<j) count the present cells that are not noise, the
 * noise cells and the begins in front of cell j; (<=j) includes j.
 * Encoder row.  The present cells that are not noise, in cell order, with a run's sentinel standing where the run begins: cell j's output
 * position is keep(<j) + begins(<j); a kept cell puts its id there, a begin its run's sentinel.  ne = keep + begins <= row_len, so
 * enc_len = row_len always suffices.  Cells [ne, enc_len) get pad_id.
 * Decoder row.  For every run in order its sentinel and then the ids of its cells; then eos_id when eos_id >= 0.  A noise cell's position is
 * noise(<j) + begins(<=j), a sentinel's noise(<j) + begins(<j).  nd = noise + begins + (eos_id >= 0) <= row_len + 2.  Cells [nd, dec_len) get
 * ignore_label, so the decoder row is a label tensor as it stands.
 * Source-cell planes.  d_enc_cell_out [rows_cap * enc_len] and d_dec_cell_out [rows_cap * dec_len] hold the cell j a copied id came from, and
 * -1 at a sentinel, at the eos and in the padding.  With them a caller gathers any other plane of the input rows (segment ids, positions, byte
 * offsets) into the new layout with one gather; this call needs no "companion planes" form.
 * Counts.  d_enc_count_out[r] = ne and d_dec_count_out[r] = nd, the UNTRUNCATED lengths; d_span_count_out[r] = the number of runs kept
 * (min(runs, max_sentinels)).  [rows_cap] int32 each.
 * Truncation.  An output position at or past enc_len / dec_len is not written.  A row that loses a cell this way (ne > enc_len or
 * nd > dec_len), in an output the caller takes, sets BfLastStatus bit 0.  The call clears the status word first, like every batch call.
 * NULL outputs.  Any of the seven outputs may be NULL; all seven NULL with rows_cap > 0 is BF_E_ARG.  enc_len is looked at only when d_enc_out
 * or d_enc_cell_out is taken, dec_len only when d_dec_out or d_dec_cell_out is.
 * Overlap.  No output may overlap d_rows, d_mask or d_seg (there is no in-place form): the compaction writes in front of cells that other lanes
 * still read.  The call does not detect it.
 * BF_E_ARG for row_len, enc_len (when used) or dec_len (when used) outside 1 .. 1 << 20; a negative rows_cap; a NULL d_rows with
 * rows_cap > 0; nspecial outside 0 .. BF_MLM_MAX_SPECIAL or a NULL special_ids with nspecial > 0; start_prob outside [0, 1] (a NaN is);
 * anything but 1 <= len_lo <= len_hi <= 1 << 20; max_sentinels outside 1 .. 1 << 20; sentinel_first or the last sentinel
 * sentinel_first + (max_sentinels - 1) * sentinel_step (computed in 64 bits) outside [0, INT32_MAX]; a NULL ModelPtr (any live handle serves).
 * The call has no workspace: it allocates nothing, with and without BfReserve.  It enqueues on `stream`, does not synchronise, reads nothing
 * back and returns 0 or BF_E_*.  Every pointer needs only the natural alignment of its type.  The result depends on (seed, r, epoch) and the
 * row alone: not on the grid, the number of rows or the order of calls.  A wave shares a row (a power-of-two slice of a wave when
 * row_len <= 32) and walks it once, in chunks of as many cells.
 * Not here: geometric span lengths; spans aligned to whole words; a host-buffer form; decoder_input_ids (the right shift is the model's);
 * T5's exact-count noise mask (it needs a random partition of the row, which is a sequential shuffle). */
BF_API int RowsDenoiseBatchDevice(void *ModelPtr, const int32_t *d_rows, int row_len, int64_t rows_cap, const int64_t *d_nrows,
                           const uint8_t *d_mask, const int32_t *d_seg, int nspecial, const int32_t *special_ids,
                           double start_prob, int len_lo, int len_hi, int sentinel_first, int sentinel_step, int max_sentinels,
                           int eos_id, int pad_id, int ignore_label, uint64_t seed, uint32_t epoch,
                           int enc_len, int32_t *d_enc_out, int32_t *d_enc_cell_out, int32_t *d_enc_count_out,
                           int dec_len, int32_t *d_dec_out, int32_t *d_dec_cell_out, int32_t *d_dec_count_out,
                           int32_t *d_span_count_out, void *stream);

/* additive (no counterpart in the reference; this comment is the specification): PACKED rows -- several sequences share a row, a segment
 * plane keeps a model's attention block-diagonal and a position plane restarts at every sequence.  Where IdsToRowsBatch pads every sequence
 * to a row of its own, this fills rows greedily and in order.
 * Units.  Sequence q of nseq = ids[off[q] .. off[q+1]), n_q ids; a range outside [0, ids_len] or with decreasing offsets is read as empty and
 * sets BfLastStatus bit 3, exactly as in IdsToRowsBatchDevice.  lead = (cls_id >= 0), trail = (sep_id >= 0), body = row_len - lead - trail.
 * Unit q is [cls_id] ids[0 .. k_q) [sep_id] with k_q = min(n_q, body): a sequence longer than a row is truncated silently, like
 * max_rows_per_seq = 1 of IdsToRowsBatch (callers who need windows use that call).  Its width is w_q = lead + k_q + trail, 0 <= w_q <= row_len.
 * A unit is never split across rows.  An empty sequence contributes only its specials; without specials its unit has width 0.
 * Rows.  With W[q] = w_0 + ... + w_{q-1} (int64, W[0] = 0): row 0 starts at sequence f[0] = 0; a row that starts at sequence s holds the
 * sequences [s, next(s)), next(s) = max{ e in (s, nseq] : W[e] - W[s] <= row_len }, and the next row starts at next(s); R is the number of rows
 * until the chain reaches nseq.  So next(s) > s always; units of width 0 stay in the row in front of them; every row but row 0 begins with a unit
 * of positive width; nseq > 0 gives R >= 1 even when every unit has width 0 (one row of padding); nseq = 0 gives R = 0; and a row that is
 * neither the last nor followed only by units of width 0 cannot take the next unit (greedy maximality).
 * Cells of row r.  Cell j < W[f[r+1]] - W[f[r]] belongs to unit q = the last q in [f[r], f[r+1]) with W[q] - W[f[r]] <= j, at place
 * x = j - (W[q] - W[f[r]]) of the unit.  rows: cls_id at x = 0 when lead, sep_id at x = w_q - 1 when trail, else ids[off[q] + x - lead].
 * seg: q - f[r] + 1 -- 1-based within the row, units of width 0 are counted, so f[r] + seg - 1 is the sequence.  pos: x.  Every cell behind the
 * last unit is padding: rows = pad_id, seg = 0, pos = 0 (a mask is seg != 0).  Padding is always on the right.
 * Per-row and per-sequence outputs.  d_row_first_seq_out[rows_cap + 1] holds f[r] for r = 0 .. min(R, rows_cap), with f[R] = nseq: the last
 * entry written is nseq when every row fit (with nseq = 0 that is entry 0).  d_seq_row_out[nseq] is the row of sequence q, d_seq_col_out[nseq]
 * is W[q] - W[f[row]], the cell where its unit begins; both are complete whatever rows_cap is.  d_nrows_out[1] is R.
 * BF_E_ARG for row_len outside 1 .. 1 << 20, body < 1, flags != 0 (the flag word is reserved), nseq < 0 or nseq > INT32_MAX, rows_cap < 0,
 * ids_len < 0, a NULL ModelPtr (any live handle of any kind serves, as for IdsToRowsBatch: it lends its device, workspaces and status word),
 * a NULL d_id_offsets or d_nrows_out, and a NULL d_ids with ids_len > 0.
 * Device form: every output but d_nrows_out may be NULL; with the three planes and d_row_first_seq_out all NULL it is a size query.  No row
 * r >= rows_cap of any plane is written, no entry past min(R, rows_cap) of d_row_first_seq_out; rows dropped that way from an output the caller
 * takes set BfLastStatus bit 0 (the call clears the status word first).  It enqueues on `stream` (a hipStream_t), does not synchronise and
 * returns 0 or BF_E_*.  After BfReserve(h, max_docs >= nseq, ...) it allocates nothing.  The kernels it launches depend on nseq and on which
 * outputs are taken, never on the data (the row starts are found by ceil(log2(nseq + 1)) rounds of pointer doubling over the whole batch, not
 * by a walk), and nothing is read back.  Every pointer needs only the natural alignment of its type;
 * planes that are all aligned to 16 bytes, with row_len % 4 == 0, take the wide stores.
 * Host form: stages the ids like IdsToRowsBatch (it reads them from id_offsets[0] to the largest offset; id_offsets[0] < 0 = BF_E_ARG) and
 * returns R.  With all four row outputs (rows, seg, pos, row_first_seq) NULL it is a size query, whatever rows_cap is; otherwise, when
 * R > rows_cap, it returns BF_E_CAPACITY with seq_row_out / seq_col_out complete and nothing else written. */
BF_API int IdsToPackedRowsBatchDevice(void *ModelPtr, const int32_t *d_ids, int64_t ids_len, const int64_t *d_id_offsets, int64_t nseq,
                               int row_len, int cls_id, int sep_id, int pad_id, int flags,
                               int32_t *d_rows_out, int32_t *d_seg_out, int32_t *d_pos_out, int32_t *d_row_first_seq_out, int64_t rows_cap,
                               int32_t *d_seq_row_out, int32_t *d_seq_col_out, int64_t *d_nrows_out, void *stream);
BF_API int64_t IdsToPackedRowsBatch(void *ModelPtr, const int32_t *ids, const int64_t *id_offsets, int64_t nseq,
                             int row_len, int cls_id, int sep_id, int pad_id, int flags,
                             int32_t *rows_out, int32_t *seg_out, int32_t *pos_out, int32_t *row_first_seq_out, int64_t rows_cap,
                             int32_t *seq_row_out, int32_t *seq_col_out);

/* additive (no counterpart in the reference; this comment is the specification): COMPANION PLANES for packed rows -- what IdsToRowsPlanesBatch
 * is to IdsToRowsBatch: up to BF_ROWS_MAX_PLANES int32 arrays that run parallel to the ids (the tokenizer's starts and ends, per-token labels, word
 * indices, ...) are gathered into int32 planes of [rows_cap * row_len] cells with the layout of d_rows_out, in the same call.  Element i of a
 * source belongs to d_ids[i].
 * IdsToPackedRowsPlanesBatchDevice / IdsToPackedRowsPlanesBatch take every argument of IdsToPackedRowsBatchDevice / IdsToPackedRowsBatch, with the
 * same meaning, checks, status bits and capacity rules, and behind them (Device form: in front of `stream`): nplanes, d_src, fill, d_planes_out
 * -- three HOST arrays of nplanes entries whose values travel to the kernel by value, exactly as in IdsToRowsPlanesBatchDevice (d_src[k] and
 * d_planes_out[k] are device pointers in the Device form, host pointers in the host form).  d_planes_out[k] may be NULL: that plane is skipped.
 * Cells.  In plane k, a cell that holds id number i of its sequence q (unit q at place x = lead + i, in the terms above) gets
 * src[k][off[q] + i]; only i < k_q is read, what a row truncates is not.  A cell that holds cls_id, sep_id or padding gets fill[k].
 * Reads and writes.  src[k] is read for at most ids_len elements, and only at cells that hold an id; a sequence read as empty (BfLastStatus
 * bit 3) has no id cells.  No row r >= rows_cap of a plane is written.  Rows dropped from a plane the caller takes set BfLastStatus bit 0,
 * also when d_rows_out, d_seg_out, d_pos_out and d_row_first_seq_out are all NULL.
 * The calls are supersets of the base calls: rows, seg, pos, row_first_seq, seq_row, seq_col and nrows are byte for byte what the base call
 * writes for the same arguments; with nplanes = 0 the call IS the base call, with the launches of the base call; a size query is the four row
 * outputs and every plane NULL.
 * BF_E_ARG for nplanes outside 0 .. BF_ROWS_MAX_PLANES, a NULL fill or d_planes_out with nplanes > 0, a NULL d_src or d_src[k] with
 * ids_len > 0 (host form: with any id to read), and for whatever the base call refuses.
 * The Device form allocates nothing after BfReserve(h, max_docs >= nseq, ...), with planes or without: it has no workspace of its own, one
 * kernel behind the base call's reads what that call left in the handle's workspaces.  Every pointer needs only the natural alignment of its
 * type: with row_len % 4 == 0 and every taken plane aligned to 16 bytes a lane makes one 16-byte store per plane, otherwise it writes one cell;
 * the sources are read element by element, because a sequence starts anywhere.
 * Host form: each source is staged beside the ids (read, like them, from id_offsets[0] to the largest offset), and the call makes the base
 * host form's two passes; when R > rows_cap with a row output or a plane taken it returns BF_E_CAPACITY with seq_row_out / seq_col_out complete
 * and nothing else written.
 * Units across sequences (whole-word masking, RowsMlmMaskBatchDevice over two planes of token offsets).  With at least one of cls_id / sep_id
 * present two units of a row are separated by a special; with that special among special_ids its cell is not eligible, so no unit of the MLM
 * call spans two sequences.  Without any special two sequences can be byte-adjacent by accident -- one ends at byte 2 of its document, the next
 * starts at byte 3 of its own behind a byte-order mark -- and their cells then join into one unit: the planes here do nothing about that, and
 * the MLM kernel's unit rule does not look at the segment plane. */
BF_API int IdsToPackedRowsPlanesBatchDevice(void *ModelPtr, const int32_t *d_ids, int64_t ids_len, const int64_t *d_id_offsets, int64_t nseq,
                                     int row_len, int cls_id, int sep_id, int pad_id, int flags,
                                     int32_t *d_rows_out, int32_t *d_seg_out, int32_t *d_pos_out, int32_t *d_row_first_seq_out, int64_t rows_cap,
                                     int32_t *d_seq_row_out, int32_t *d_seq_col_out, int64_t *d_nrows_out,
                                     int nplanes, const int32_t *const *d_src, const int32_t *fill, int32_t *const *d_planes_out, void *stream);
BF_API int64_t IdsToPackedRowsPlanesBatch(void *ModelPtr, const int32_t *ids, const int64_t *id_offsets, int64_t nseq,
                                   int row_len, int cls_id, int sep_id, int pad_id, int flags,
                                   int32_t *rows_out, int32_t *seg_out, int32_t *pos_out, int32_t *row_first_seq_out, int64_t rows_cap,
                                   int32_t *seq_row_out, int32_t *seq_col_out,
                                   int nplanes, const int32_t *const *src, const int32_t *fill, int32_t *const *planes_out);

/* additive (no counterpart in the reference; this comment is the specification): STREAM rows -- "concatenate and chunk", the input of causal-LM
 * pretraining: every sequence closed by its specials, all of them laid end to end, the stream cut into rows of exactly row_len cells, with
 * next-token labels, a segment plane and a position plane.  Where IdsToPackedRowsBatch truncates a sequence longer than a row and never splits
 * one, here a sequence runs over a row's edge into the next row: nothing is truncated, and nothing is padded but the tail of the last row.
 * Units.  Sequence q of nseq = ids[off[q] .. off[q+1]), n_q ids; a range outside [0, ids_len] or with decreasing offsets is read as empty and
 * sets BfLastStatus bit 3, exactly as in IdsToRowsBatchDevice; a sequence of more than INT32_MAX - 2 ids is read the same way (the widths are
 * int32 like every count the scan takes).  lead = (bos_id >= 0), trail = (eos_id >= 0).  Unit q is [bos_id] ids[0 .. n_q) [eos_id], every id
 * and none dropped, of width w_q = lead + n_q + trail.  W is the int64 exclusive scan of the widths, T = W[nseq] the length of the stream S,
 * the units laid end to end.
 * Rows.  Row r is S[r * L .. (r+1) * L), L = row_len.  R = ceil(T / L); with flags bit 0 ("drop the last incomplete row") R = floor(T / L).
 * T = 0 gives R = 0: that is nseq = 0, and also every unit of width 0 (the packed call writes one row of padding there; this call does not).
 * Cells.  Cell j of row r is stream position t = r * L + j.  For t < T: q = the last q in [0, nseq) with W[q] <= t -- units of width 0 share
 * their W with the unit behind them, so this is the unit the cell lies in -- and x = t - W[q].  rows: bos_id at x = 0 when lead, eos_id at
 * x = w_q - 1 when trail, else ids[off[q] + x - lead].  seg: q - f[r] + 1, where f[r] is the unit of cell 0 of the row (it always has positive
 * width); units of width 0 are counted, so f[r] + seg - 1 is the sequence, as in the packed call, and a unit that continues from the row before
 * has seg 1.  pos: x, the position within the unit, continuing across rows; with flags bit 1 pos = min(x, j): a unit that continues from the
 * row before counts from the row's edge (what a model needs whose attention is confined to the row and the segment).  labels: with t + 1 < T,
 * S[t + 1] -- the stream's next element, which may be a special, and for j = L - 1 is the next row's first: it is taken from the stream, whether
 * or not that row is written; with flags bit 2 a label whose t + 1 lies in another unit than t is ignore_label; with t + 1 = T, ignore_label.
 * t >= T is padding, always on the right of the last row: rows = pad_id, seg = 0, pos = 0, labels = ignore_label.
 * Per-row outputs, [rows_cap] int32 each: d_row_first_seq_out[r] = f[r], d_row_first_pos_out[r] = r * L - W[f[r]].
 * Per-sequence outputs, [nseq] int32 each: d_seq_row_out[q] = W[q] / L and d_seq_col_out[q] = W[q] mod L, the cell where the unit begins.  They
 * are complete whatever rows_cap and flags bit 0 are; a row >= R is a legitimate answer (a unit in the dropped tail, or units of width 0
 * behind the last cell when L divides T).
 * Counts.  d_nrows_out is int64[2] = {R, T}, and required; its first entry serves as the d_nrows of RowsMlmMaskBatchDevice and its relatives.
 * Example: ids = 1000 .. 1009, off = [0,3,3,3,10], L = 4, bos 1, eos 2, pad 0, flags 0: T = 18, R = 5,
 *   rows = [1 1000 1001 1002] [2 1 2 1] [2 1 1003 1004] [1005 1006 1007 1008] [1009 2 0 0]
 *   seg  = [1 1 1 1] [1 2 2 3] [1 2 2 2] [1 1 1 1] [1 1 0 0]        pos = [0 1 2 3] [4 0 1 0] [1 0 1 2] [3 4 5 6] [7 8 0 0]
 *   labels: row 0 = [1000 1001 1002 2], the last row = [2 -100 -100 -100] (ignore_label -100)
 *   row_first_seq = [0 0 2 3 3], row_first_pos = [0 4 1 3 7], seq_row = [0 1 1 2], seq_col = [0 1 3 1].
 * BF_E_ARG for row_len outside 1 .. 1 << 20 (there is no body >= 1 condition: L = 1 with both specials is fine, since units split), a flag bit
 * above 2, nseq < 0 or nseq > INT32_MAX, rows_cap < 0, ids_len < 0, ceil((ids_len + (lead + trail) * nseq) / row_len) > INT32_MAX (the
 * host-known bound of R: seq_row is int32), a NULL ModelPtr (any live handle of any kind serves), a NULL d_id_offsets or d_nrows_out, and a
 * NULL d_ids with ids_len > 0.
 * Device form: every output but d_nrows_out may be NULL; the six row outputs (rows, seg, pos, labels, row_first_seq, row_first_pos) all NULL is
 * a size query.  No row r >= rows_cap of any row output is written; rows dropped that way from an output the caller takes set BfLastStatus
 * bit 0.  The call clears the status word first, enqueues on `stream` (a hipStream_t), does not synchronise, reads nothing back and returns 0
 * or BF_E_*.  The kernels it launches depend on nseq and on which outputs are taken, never on the data.  After BfReserve(h, max_docs >= nseq,
 * ...) it allocates nothing: it has no workspace beyond the widths, block sums and W of the packed call, and none sized by the row count (R is
 * not bounded by nseq here).  Every pointer needs only the natural alignment of its type; row_len % 4 == 0 with every taken plane aligned to
 * 16 bytes takes the 16-byte stores.
 * Host form: it stages the ids like IdsToPackedRowsBatch (id_offsets[0] < 0 = BF_E_ARG), makes two passes and returns R.  The six row outputs
 * all NULL is a size query, whatever rows_cap is; otherwise R > rows_cap returns BF_E_CAPACITY with seq_row_out / seq_col_out complete and
 * nothing else written.
 * Not here: overlapping rows, companion planes, shuffling, and a cap on the ids of a document (the tokenizer call's max_ids_per_doc is that). */
BF_API int IdsToStreamRowsBatchDevice(void *ModelPtr, const int32_t *d_ids, int64_t ids_len, const int64_t *d_id_offsets, int64_t nseq,
                               int row_len, int bos_id, int eos_id, int pad_id, int ignore_label, int flags,
                               int32_t *d_rows_out, int32_t *d_seg_out, int32_t *d_pos_out, int32_t *d_labels_out,
                               int32_t *d_row_first_seq_out, int32_t *d_row_first_pos_out, int64_t rows_cap,
                               int32_t *d_seq_row_out, int32_t *d_seq_col_out, int64_t *d_nrows_out, void *stream);
BF_API int64_t IdsToStreamRowsBatch(void *ModelPtr, const int32_t *ids, const int64_t *id_offsets, int64_t nseq,
                             int row_len, int bos_id, int eos_id, int pad_id, int ignore_label, int flags,
                             int32_t *rows_out, int32_t *seg_out, int32_t *pos_out, int32_t *labels_out,
                             int32_t *row_first_seq_out, int32_t *row_first_pos_out, int64_t rows_cap,
                             int32_t *seq_row_out, int32_t *seq_col_out);

/* reference tokdll:1669-1679 */
BF_API int SetNoDummyPrefix(void *ModelPtr, bool fNoDummyPrefix);

/* reference tokdll:818-911 (blingfiretokdll.def: WordHyphenationWithModel) over FAHyphInterpreter_core_t.h:136-267: the word with uHy
 * written behind every character that a pattern of the model's [w2h] section (syllab.bin) marks as a hyphenation point.  hModel: a LoadModel
 * handle of a model with a [w2h] section; any other handle, and NULL, answer -1 (the reference has no built-in model here).  Returns 0
 * for a 0-byte input; -1 for a negative size, a NULL string, invalid UTF-8 within the first 300 characters or a uHy that UTF-8 cannot
 * encode (negative, a surrogate, above U+10FFFF); otherwise the bytes the whole output needs, plus 1 for a terminating 0 that is written
 * and counted only when it fits.  At most 300 characters are looked at (FALimits::MaxWordSize), a leading BOM is not part of the word,
 * U+0000 is written as U+0020.  Whole symbols are copied while they fit MaxOutUtf8StrByteCount; pOutUtf8Str may be NULL to size only.
 * Runs as a batch of one on the GPU (the kernels of WordHyphenationBatch). */
BF_API int WordHyphenationWithModel(const char *pInUtf8Str, int InUtf8StrByteCount, char *pOutUtf8Str, const int MaxOutUtf8StrByteCount,
                             void *hModel, const int uHy);
/* additive: WordHyphenationWithModel (tokdll:818-911, FAHyphInterpreter_core_t.h:136-267) for many words at once; word w =
 * text[word_offsets[w] .. word_offsets[w+1]).  The output of word w -- the bytes the single call produces, without the terminating 0;
 * nothing for a word the single call answers with 0 or -1 -- = text_out[text_offsets_out[w] .. text_offsets_out[w+1]).  Contracts of
 * TextToWordsBatch / TextToWordsBatchDevice: the host form returns the byte total, or BF_E_CAPACITY with complete offsets and text_out
 * untouched; the Device form writes only the offsets when d_text_out is NULL, never writes at or past text_cap, does not synchronise and,
 * after BfReserve(h, max_words, max_bytes, 0), does not allocate.  BF_E_ARG for a uHy the single call refuses, BF_E_UNSUPPORTED for a
 * handle without a usable [w2h] section, for the whole call.  Words whose offsets leave the text are empty (BfLastStatus bit 3). */
BF_API int64_t WordHyphenationBatch(void *ModelPtr, const char *text, const int64_t *word_offsets, int64_t nwords, char *text_out, int64_t text_cap,
                             int64_t *text_offsets_out, int uHy);
BF_API int WordHyphenationBatchDevice(void *ModelPtr, const char *d_text, const int64_t *d_word_offsets, int64_t nwords, int64_t total_bytes,
                               char *d_text_out, int64_t text_cap, int64_t *d_text_offsets_out, int uHy, void *stream);

/* ---- additive batch entry points (a GPU wants batches; semantics = "for every document,
 *      exactly what TextToIds(h, doc, len, buf, max_ids_per_doc, unk) would have written",
 *      concatenated in document order) ---- */

/* Host buffers.  text = concatenated documents; doc_offsets[ndocs+1] = byte offsets.
 * ids_out[ids_cap] receives the concatenated ids, id_offsets_out[ndocs+1] their boundaries.
 * Returns the total number of ids, or a negative error code (BF_E_*); with BF_E_CAPACITY id_offsets_out is still complete
 * (id_offsets_out[ndocs] = the ids_cap that would have sufficed).  Large batches (>= 128 MiB of text) are pipelined in chunks of
 * whole documents through page-locked staging; the call returns when everything is in the caller's arrays.
 * BPE models (gpt2.bin, roberta.bin, ...): every document has an answer, as with the reference, whose arc list is an unbounded
 * std::vector (FATokenSegmentationTools_1best_bpe_t.h:143-144,197).  A document that needs more candidate arcs than the batch
 * workspace reserves per document (e.g. nothing but one long run of '-') is tokenised by one wave out of a pool of the handle
 * (64 MiB at first, BfSetBpePoolBytes); when a batch needs more, this call grows the pool and runs again.  The ...BatchDevice form
 * cannot allocate: there such a document gets 0 ids and BfLastStatus reports bit 64 (size the pool with BfSetBpePoolBytes first). */
BF_API int64_t TextToIdsBatch(void *ModelPtr, const char *text, const int64_t *doc_offsets, int64_t ndocs,
                       int32_t *ids_out, int64_t ids_cap, int64_t *id_offsets_out,
                       int max_ids_per_doc, int unk);

/* Device buffers (all five pointers are device memory of the model's GPU).  Work is enqueued on
 * `stream` (a hipStream_t; NULL = the default stream) and the call returns without synchronising:
 * 0 = enqueued, negative = error.  The total id count is d_id_offsets_out[ndocs].  ids_cap must be
 * >= min(2 * (total_bytes + ndocs), ndocs * max_ids_per_doc) to be safe for any input (WordPiece models never
 * need more than total_bytes); ids beyond ids_cap are dropped
 * and reported by BfLastStatus.  d_text needs no padding.
 * PRECONDITION of every ...BatchDevice call: d_doc_offsets[0] == 0 and d_doc_offsets[ndocs] == total_bytes (offsets are relative to
 * d_text; pass d_text + first_byte and rebased offsets for a sub-range).  The kernels index their workspaces by these offsets; a
 * document whose range falls outside [0, total_bytes] is treated as empty and reported through BfLastStatus (bit 3).
 * Every device pointer of every ...BatchDevice call needs only the natural alignment of its element type (1 byte for text, 4 for int32_t,
 * 8 for int64_t): nothing in front of d_text or at / behind d_text + total_bytes is looked at, nothing in front of an output or at / behind
 * its capacity is written -- the contract tests/test_gpu_caller_pointers.py pins, with every pointer inside a larger buffer.
 * A handle owns ONE set of device workspaces: the ...Device calls on one handle must be ordered on the device (the same
 * stream, or streams the caller synchronises); for concurrent batches use one handle per stream (LoadModel is cheap:
 * a few MB of tables).  The host-buffer calls serialise on the handle's mutex and synchronise before they return. */
BF_API int TextToIdsBatchDevice(void *ModelPtr, const char *d_text, const int64_t *d_doc_offsets, int64_t ndocs,
                         int64_t total_bytes, int32_t *d_ids_out, int64_t ids_cap, int64_t *d_id_offsets_out,
                         int max_ids_per_doc, int unk, void *stream);

/* Batch forms of TextToIdsWithOffsets: starts_out / ends_out are parallel to ids_out (same offsets array). */
BF_API int64_t TextToIdsWithOffsetsBatch(void *ModelPtr, const char *text, const int64_t *doc_offsets, int64_t ndocs,
                                  int32_t *ids_out, int32_t *starts_out, int32_t *ends_out, int64_t cap,
                                  int64_t *id_offsets_out, int max_ids_per_doc, int unk);
BF_API int TextToIdsWithOffsetsBatchDevice(void *ModelPtr, const char *d_text, const int64_t *d_doc_offsets, int64_t ndocs,
                                    int64_t total_bytes, int32_t *d_ids_out, int32_t *d_starts_out, int32_t *d_ends_out,
                                    int64_t cap, int64_t *d_id_offsets_out, int max_ids_per_doc, int unk, void *stream);

/* additive: the byte offsets this library produces and takes (the starts / ends above, the offset planes of the row calls, the spans of
 * RowsSpanCellsBatchDevice) <-> offsets in code points (what a Python str indexes by) or UTF-16 code units (C#, JS), on the device.
 *
 * Definitions.  Document d is text[doc_off[d] .. doc_off[d+1]) and has n_d bytes; a range outside [0, total_bytes] or with decreasing offsets
 * reads as empty and sets BfLastStatus bit 3, as in every Device call.  The weight of a byte value b:
 *   unit = 0 (code points):        0 if (b & 0xC0) == 0x80, else 1;
 *   unit = 1 (UTF-16 code units):  0 if (b & 0xC0) == 0x80; 2 if b >= 0xF0; else 1.
 * The rule is on bytes alone, so it is defined for byte-level models (gpt2.bin) whose documents need not be valid UTF-8; for valid UTF-8 it
 * equals what len(doc[:i].decode()), or the UTF-16 length of the same prefix, gives.
 *   C_d(i), 0 <= i <= n_d:  the sum of the weights of the first i bytes of the document.  U_d = C_d(n_d).
 *   B_d(k), 0 <= k <= U_d:  n_d if k == U_d, else min { i : C_d(i+1) > k } -- the first byte of the character that holds unit k (an index
 *                           that points at a low surrogate maps to its character's first byte).
 * Items.  d_item_offsets is int64[ndocs+1], non-decreasing from 0 (the tokenizer's d_id_offsets_out as it stands): item i belongs to the document
 * d with off[d] <= i < off[d+1].  NULL: item d belongs to document d (one span per document, the QA form).  Items at or past
 * min(items_cap, off[ndocs]) are neither read nor written, so chaining behind a tokenizer call that overflowed its ids_cap is safe.  (An item
 * no document holds -- offsets that do not start at 0 -- gives -1 and bit 3.)
 * Ends.  flags bit 0: the input ends are exclusive (default inclusive, like the tokenizer's); flags bit 1: the output ends are exclusive (the
 * offset_mapping convention of other tokenizer libraries).  With x = e + 1 for an inclusive input end and x = e otherwise, out = F(x), minus 1
 * when the output is inclusive.  Starts: out = F(s).  F is C_d in ByteToCharOffsetsBatchDevice and B_d in CharToByteOffsetsBatchDevice.  A negative
 * input (the dummy prefix's -1, a plane's fill, "no answer") gives -1 and sets no status bit.  A non-negative argument of F beyond n_d
 * (respectively U_d) gives -1 and sets bit 3; so does an answer beyond INT32_MAX (a document of more than 2 GiB).
 * Either input / output pair may be NULL; d_doc_units_out ([ndocs], U_d; saturates at INT32_MAX) may be NULL, and it alone is a legal call.
 * d_starts_out == d_starts and d_ends_out == d_ends (in place) are allowed: a lane reads only its own element before it writes it.
 * BF_E_ARG: a unit other than 0 or 1, a flag bit above 1, negative sizes, an input without its output or an output without its input, a NULL
 * d_text with total_bytes > 0, a NULL d_doc_offsets, every output NULL with items to do, a NULL ModelPtr.  Any live handle serves: it lends its
 * device, workspaces and status word; the model is not consulted.
 * Like every batch call it clears the status word first, enqueues on `stream`, does not synchronise, reads nothing back and returns 0 or
 * BF_E_*.  The kernels it launches depend on the sizes and on which outputs are taken, never on the data.  The workspace is 28 bytes per 64 bytes
 * of text (an index over 64-byte chunks of the text buffer: two masks, a count and its 64-bit prefix sum; the one pass over the text); after
 * BfReserve(h, ..., max_bytes >= total_bytes, ...) the calls allocate nothing.  Every pointer needs only the natural alignment of its type;
 * nothing in front of d_text or at or behind d_text + total_bytes is looked at.
 * Not here: host-buffer forms (on the host this is a cumulative sum), grapheme clusters, validation of the UTF-8. */
BF_API int ByteToCharOffsetsBatchDevice(void *ModelPtr, const char *d_text, const int64_t *d_doc_offsets, int64_t ndocs, int64_t total_bytes,
                                        const int64_t *d_item_offsets, int64_t items_cap, const int32_t *d_starts, const int32_t *d_ends, int unit, int flags,
                                        int32_t *d_starts_out, int32_t *d_ends_out, int32_t *d_doc_units_out, void *stream);
BF_API int CharToByteOffsetsBatchDevice(void *ModelPtr, const char *d_text, const int64_t *d_doc_offsets, int64_t ndocs, int64_t total_bytes,
                                        const int64_t *d_item_offsets, int64_t items_cap, const int32_t *d_starts, const int32_t *d_ends, int unit, int flags,
                                        int32_t *d_starts_out, int32_t *d_ends_out, int32_t *d_doc_units_out, void *stream);

/* additive: the reference's dictionary interpreter, FADictInterpreter_t<int>::GetInfo
 * (blingfireclient.library/inc/FADictInterpreter_t.h:31-66,334-390; FAMphInterpretTools_t.h:97-122), for many keys at once over the
 * [pos-dict] of a tokenizer model (gpt2.bin, xlm_roberta_base.bin, ...) -- the same Mealy automaton / K2I / I2Info the segmenters use.
 * Key k = keys[key_offsets[k] .. key_offsets[k+1]) as int code points (the reference's Ty = int; byte-encoded models such as gpt2.bin
 * store bytes and U+2581 as their symbols), configured like blingfiretokdll would configure it (SetConf without a transformation):
 * an l2r dictionary is looked up as is (the [pos-dict] charmap is not applied, FADictInterpreter_t.h:203-205), an r2l one after
 * charmap normalisation and reversal, an ignore-case one (either direction) after folding every symbol (FAUtf32ToLower, :231-238) and
 * then the charmap.  ret_out[k] = GetInfo's return value (value count, -1 = no such key: not in the dictionary,
 * empty or longer than 300 symbols); info_ids_out[k] = GetInfoId (-1 = none); the values of key k (for the tokenizer dictionaries:
 * [token id, float score bits]) = values_out[value_offsets_out[k] .. value_offsets_out[k+1]).  ret_out / info_ids_out may be NULL.
 * Returns the total value count or BF_E_* (BF_E_CAPACITY: the offsets are valid and tell the size).  The Device form takes device
 * pointers + a hipStream_t, never writes past values_cap and returns 0 / BF_E_*; with d_values_out == NULL it only fills the
 * per-key results and the offsets. */
BF_API int64_t DictGetInfoBatch(void *ModelPtr, const int32_t *keys, const int64_t *key_offsets, int64_t nkeys, int32_t *ret_out, int32_t *info_ids_out,
                                int32_t *values_out, int64_t values_cap, int64_t *value_offsets_out);
BF_API int DictGetInfoBatchDevice(void *ModelPtr, const int32_t *d_keys, const int64_t *d_key_offsets, int64_t nkeys, int32_t *d_ret_out,
                                  int32_t *d_info_ids_out, int32_t *d_values_out, int64_t values_cap, int64_t *d_value_offsets_out, void *stream);

/* Per-kernel GPU time of the last batch call on this handle, measured with HIP events recorded on the
 * call's own stream.  Synchronises with those events.  Fills up to n floats (milliseconds):
 * [0] prep (decode+normalise+classify)  [1] tokenise (lexer / segmenter)  [2] scan  [3] compact  [4] total  [5] the dominant kernel of the
 * tokenise segment alone.  After IdsToPackedRowsBatchDevice: [0] widths + scan, [1] next + the doubling rounds, [2] the scan of the marks and the
 * per-row / per-sequence outputs, [3] the fill of the planes, [4] total, [5] the doubling rounds alone.  After IdsToPackedRowsPlanesBatchDevice with a plane taken, [3] covers the
 * fill and the kernel of the companion planes behind it.  After IdsToStreamRowsBatchDevice: [0] widths + scan, [2] the per-sequence outputs and
 * the counts, [3] the fill, [4] total ([1] and [5] are 0).  After ByteToCharOffsetsBatchDevice / CharToByteOffsetsBatchDevice: [0] the index pass
 * over the text, [2] the scan of the chunk counts, [3] the per-document and the per-item kernel, [4] total ([1] and [5] are 0).
 * Returns the number of values written, or a negative error. */
BF_API int BfLastKernelMs(void *ModelPtr, float *ms, int n);

/* Status word of the last batch call on this handle (synchronises).  It is that call's OWN: every batch call that takes a handle -- the
 * tokenizer calls, words and sentences, the row, pair-row, plane, packed, stream, span-cell, MLM and denoise calls, ByteToCharOffsetsBatchDevice
 * and CharToByteOffsetsBatchDevice, IdsToText, DictGetInfo and WordHyphenation, Device and host forms alike, and the single-document calls, which are batches of one -- clears the word when it begins,
 * on its stream, so nothing an earlier call reported survives it, whatever the order of the calls (tests/test_gpu_call_order.py runs every
 * ordered pair of them on one handle).  A call of the two-pass kind reports what its size pass found; a call that was refused with BF_E_ARG
 * or BF_E_UNSUPPORTED before it enqueued anything leaves the word alone.  NormalizeSpacesBatch and TextToHashesBatch take no handle and have
 * no status.
 * 0 = ok; bit 0 (1) = ids_cap / rows_cap overflow (RowsDenoiseBatchDevice: a row longer than enc_len / dec_len); bit 1 (2) and bit 4 (16) = an internal
 * limit the load-time checks exclude was met (the results of the batch are not to be trusted; the host-buffer calls return
 * BF_E_INTERNAL); bit 2 (4) = IdsToText: a sequence held an id the model does not know and yields no text; bit 3 (8) = a document's byte
 * range was outside [0, total_bytes] (Device calls: see the precondition above) and was treated as empty (the row calls: an id range outside
 * [0, ids_len]; the span cells: a row whose item is out of range; the offset conversions: also a position beyond its document).  Per-document, the rest of the batch is valid: bit 5 (32) = a BPE document on which the reference itself does not
 * terminate (a skipped start position left without an arc, FATokenSegmentationTools_1best_bpe_t.h:299-313) got 0 ids; bit 6 (64) = a
 * BPE document's arcs did not fit the pool and it got 0 ids (only the ...BatchDevice forms: the host-buffer calls grow the pool and
 * run again; BfSetBpePoolBytes). */
BF_API int BfLastStatus(void *ModelPtr);

/* Last load error message of the calling thread ("" if none). */
BF_API const char *BfLastError(void);

/* Model facts: 0 = WordPiece lexer, 1 = Unigram-LM, 2 = BPE, 3 = BPE-opt, 4 = BPE with merge ranks, 5 = [i2w] only (IdsToText),
 * 6 = [w2h] only (WordHyphenation; a model that has [w2h] beside other sections keeps its kind and hyphenates too) */
BF_API long long BfBpeFallbackDocs(void *ModelPtr);   /* diagnostics: documents of the last BPE batch that took the full (sort + apply) path */
BF_API int BfModelKind(void *ModelPtr);

/* Optional: size every workspace of the handle for batches of up to max_docs documents / max_bytes bytes of text now, so that
 * later ...BatchDevice calls of that size allocate nothing, the first one included (workspaces only ever grow; growing means hipMalloc,
 * which synchronises the device and is not allowed inside a stream capture).  want_offsets != 0 also sizes the offsets API.
 * Every kind of handle has the workspaces of IdsToRowsBatchDevice and IdsToPairRowsBatchDevice (the same ones) and those of
 * IdsToPackedRowsBatchDevice (about 36 bytes per sequence) sized for max_docs sequences or pairs (an [i2w]-only handle has no others).
 * The packed stage's workspaces also cover IdsToPackedRowsPlanesBatchDevice (one kernel behind the base call's, over what that call left
 * there) and IdsToStreamRowsBatchDevice (the widths, block sums and W; nothing of it is sized by the row count, which max_docs does not
 * bound).  RowsSpanCellsBatchDevice, RowsMlmMaskBatchDevice, RowsMlmPredictionsBatchDevice and RowsDenoiseBatchDevice have no workspace:
 * they allocate nothing on any handle, reserved or not.  (tests/test_gpu_reserve_contract.py counts the allocations around every one of these.)
 * Every kind of handle also gets the index of ByteToCharOffsetsBatchDevice / CharToByteOffsetsBatchDevice, sized from max_bytes alone (28 bytes per
 * 64 bytes of text, and the scan's block sums for that many chunks): after that the two calls allocate nothing, the first one included.
 * That is 0.44 bytes of HBM per byte of max_bytes on EVERY reserved handle, whether it ever converts an offset or not (about 2.2 GB for a
 * reserve of 5.1 GB of text): count it when sizing HBM.  A handle that is not reserved allocates the index in its first conversion call.
 * A WordPiece handle also gets the buffers of TextToWordsBatchDevice / TextToSentencesBatchDevice (12 bytes per byte of text and 8 per
 * document); a handle with a [pos-dict] gets its lookup tables uploaded and the workspaces of DictGetInfoBatchDevice for max_docs keys; a
 * handle with [w2h] those of WordHyphenationBatchDevice for max_docs words.
 * The limits of the promise:
 *  - one workspace is left out: the long-document workspace of the words modes (40 .. 56 bytes per cell, about one cell per byte of text).
 *    It is sized for the worst case from the batch's size alone, before any kernel has looked for a long document: with the default
 *    knobs EVERY first TextToWordsBatchDevice / TextToSentencesBatchDevice call of a given size (documents, bytes) allocates it, whatever
 *    its documents look like -- a batch of uniform short lines too -- and every later call of a larger size allocates it again.  Such
 *    calls are not safe inside a stream capture.  The only way to avoid the allocation today is the no_long knob of BfSetVariant
 *    (bit 30, 0x40000000; bf_internal.h), which keeps every document on one lane;
 *  - it holds for the BfSetVariant value and the BfSetBpePoolBytes size in force when BfReserve was called (the workspaces are those of the
 *    program these select): after either call, call BfReserve again;
 *  - the built-in models of the words calls (ModelPtr == NULL there) have no handle a caller could reserve: load wbd.bin / sbd.bin and pass
 *    the handle.
 * Returns 0 or BF_E_*. */
BF_API int BfReserve(void *ModelPtr, int64_t max_docs, int64_t max_bytes, int want_offsets);
/* BPE models: the size of the pool from which documents with very many candidate arcs claim their working memory (about 16 bytes per
 * arc: a run of 10^6 identical characters whose run lengths are vocabulary entries takes ~350 MB).  Takes effect with the next batch
 * (the pool only grows).  Returns the previous size or BF_E_*. */
BF_API int64_t BfSetBpePoolBytes(void *ModelPtr, int64_t bytes);

/* Multi-GPU (SURVEY.md section 8b "SetDevices", 8e): range-shards the HOST-buffer batch calls of this handle (TextToIdsBatch,
 * TextToIdsWithOffsetsBatch) over n devices of this node.  The tables are replicated on every listed device; a batch is split into
 * n contiguous, byte-balanced document ranges (BfShardRanges), each tokenised by a host thread of its own on its own device, stream set
 * and workspace; ids and offsets come back exactly as one device would have returned them (no collective: documents are independent).
 * A device may be listed more than once (logical shards on one device).  BfSetDevices(h, &own_device, 1) ends sharding.
 * The ...BatchDevice calls (their buffers live on ONE device) and the single-document calls stay on the handle's own device; a caller
 * that keeps its shards resident on the devices itself takes the per-range handles with BfShardHandle(h, g) (NULL past the last range;
 * owned by h, released by FreeModel(h) / the next BfSetDevices) and calls TextToIdsBatchDevice on each from a thread of its own.
 * Reference semantics preserved per document: blingfiretokdll.cpp:1619-1646.  Returns 0 or BF_E_*. */
BF_API int BfSetDevices(void *ModelPtr, const int *device_ids, int n);
BF_API void *BfShardHandle(void *ModelPtr, int g);
/* the ranges a batch is split into over G devices: bounds[0 .. G], range g = documents [bounds[g], bounds[g + 1]): bounds[g] is the
 * document boundary closest to g / G of the text (pure host arithmetic, no device needed) */
BF_API int BfShardRanges(const int64_t *doc_offsets, int64_t ndocs, int G, int64_t *bounds);

#define BF_E_ARG      (-1)   /* bad argument */
#define BF_E_DEVICE   (-2)   /* HIP error */
#define BF_E_CAPACITY (-3)   /* ids_cap too small */
#define BF_E_INTERNAL (-4)   /* internal capacity exceeded */
#define BF_E_UNSUPPORTED (-5)

#ifdef __cplusplus
}
#endif
#endif
