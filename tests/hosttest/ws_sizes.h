// ws_sizes.h -- TEST-ONLY: the sizes, in ELEMENTS, of the workspaces that blingfire_amd/csrc/bf_capi.cpp reserves for a batch of ndocs documents and
// total_bytes bytes (reserve_ids_workspaces, reserve_flat_workspaces, reserve_sp_workspaces, reserve_w2h_workspaces), RESTATED here line by line so
// that the host emulators allocate what the product allocates and no more: a program that writes past it is an access outside the block under the
// sanitizers (tests/test_sanitized_host.py).  A restatement, not shared code: a size that changes in bf_capi.cpp has to change here too.
#pragma once
#include <stdint.h>

namespace bfa {

// staged ids of the _wp programs (bf_wave.h wv_ids_slot; int32 each: w_tmp) and their spans (two int32 each: w_span)
inline int64_t ws_tmp_cells(int64_t ndocs, int64_t total_bytes) { return total_bytes + 8 * ndocs + 64; }
// one cell per document and one more: counts, entry counts and offsets, document states, lists, flags, stream lengths
inline int64_t ws_doc_cells(int64_t ndocs) { return ndocs + 1; }
// the flat program (bf_flat.h): entries, homes, entry spans (one cell per byte; the homes' spans: two); word records of 16 bytes (record_shift =
// bf_flat_key.h WF_REC_SHIFT); the range table (int64 each) and the two list lengths of every range behind the records (int32 each)
inline int64_t ws_flat_cells(int64_t total_bytes) { return total_bytes + 64; }
inline int64_t ws_flat_records(int64_t total_bytes, int record_shift) { return (total_bytes >> record_shift) + 64; }
inline int64_t ws_flat_range_cells(int64_t nranges) { return nranges + 2; }
// _sp: stream elements over all documents (slot of document d = mul * (doc_off[d] + d), mul = 2 with a charmap): the element stream (uint16, read up
// to ws_sp_stream_slack elements past it by the sector buffers of the Unigram lane program), staged ids (the larger of this and ws_tmp_cells), spans
inline int64_t ws_sp_cells(int mul, int64_t ndocs, int64_t total_bytes) { return (int64_t)mul * (total_bytes + ndocs) + 64; }
constexpr int64_t ws_sp_stream_slack = 256;
inline int64_t ws_sp_tmp_cells(int mul, int64_t ndocs, int64_t total_bytes) { const int64_t a = ws_sp_cells(mul, ndocs, total_bytes), b = ws_tmp_cells(ndocs, total_bytes); return a > b ? a : b; }
// the BPE wave program's scratch (six uint32 per stream cell for a word of more than 64 arcs) = the element workspace of k_bpe_seg (w_s1)
inline int64_t ws_bpe_scratch_words(int64_t sp_cells) { return sp_cells * 6 + 64; }
// the hyphenator's position stream (bf_w2h.h w2h_slot; uint16 each: w_hcls)
inline int64_t ws_w2h_cells(int64_t nwords, int64_t total_bytes) { return total_bytes + 2 * nwords + 64; }

} // namespace bfa
