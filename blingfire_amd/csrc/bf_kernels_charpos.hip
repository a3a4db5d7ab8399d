// bf_kernels_charpos.hip -- byte offsets <-> character offsets over text that is on the device (bf_charpos.h has the lane code and the
// definitions; include/blingfiretokdll_amd.h ByteToCharOffsetsBatchDevice is the specification).
//
//  k_char_index   the only pass over the text.  A wave takes 1024 consecutive bytes of the batch's text buffer, a lane 16 of them in one load
//                 (the text needs no alignment: the load is a 16-byte load at a byte address; the one lane that holds the text's end reads byte
//                 by byte and takes the bytes at or past total_bytes as continuation bytes, without loading them).  A lane turns its four words
//                 into 16 bits of each mask; two exchanges with the lanes 1 and 2 away put four pieces together, and the first lane of every four
//                 writes the chunk's masks and its weight: 16 chunks per wave, 128 consecutive bytes per store.  Chunks ignore the documents.
//  (scan)         k_scan_* of bf_kernels_sp.hip over the chunk weights -> P (int64, nchunks + 1 entries).
//  k_char_docs    lane per document: a range outside the text sets status bit 3; U_d where the caller takes it.
//  k_char_fwd     lane per item.  The documents of a wave's first and last item are found by the wave together in the item offsets (64 probes
//  k_char_inv     a round, bf_stream.h), a lane finds its own between the two.  Forward: two G evaluations per position.  Inverse: a binary search
//                 of P over the document's chunks, then six halvings inside one chunk's masks.  A lane reads its own element before it writes it,
//                 so the outputs may be the inputs.  Items at or past min(items_cap, off[ndocs]) are neither read nor written.
// No lane walks a document, no LDS, no atomics but the status word's.
#include "bf_kernels_common.h"

namespace bfa {

__global__ __launch_bounds__(256) void k_char_index(CharposParams p)
{
    const int lane = lane_id();
    const int64_t tiles = (p.total_bytes + CHARPOS_WAVE_BYTES - 1) / CHARPOS_WAVE_BYTES;
    for (int64_t tile = (int64_t)blockIdx.x * 4 + wave_in_block(); tile < tiles; tile += (int64_t)gridDim.x * 4) {
        const int64_t at = tile * CHARPOS_WAVE_BYTES + lane * CHARPOS_LANE_BYTES;
        uint32_t w[4] = {0x80808080u, 0x80808080u, 0x80808080u, 0x80808080u};
        // A 16-byte copy from a byte pointer: one global_load_dwordx4 at the byte address, because the amdhsa target compiles with unaligned access
        // allowed (its default; the hardware takes the address).  It stays correct under a build that forbids unaligned access (the compiler then
        // splits the copy into byte loads), but sixteen times the load instructions: check the listing after a change of the build flags.
        if (at + CHARPOS_LANE_BYTES <= p.total_bytes) __builtin_memcpy(w, p.text + at, CHARPOS_LANE_BYTES);
        else if (at < p.total_bytes) charpos_tail_words(p.text, at, p.total_bytes, w);
        uint32_t lead16, four16;
        charpos_piece(w, &lead16, &four16);
        unsigned long long lead = charpos_place(lead16, lane), four = p.four ? charpos_place(four16, lane) : 0;
        lead |= __shfl_xor(lead, 1, 64); lead |= __shfl_xor(lead, 2, 64);
        if (p.four) { four |= __shfl_xor(four, 1, 64); four |= __shfl_xor(four, 2, 64); }      // (uniform: no lane is missing from an exchange)
        const int64_t c = tile * (CHARPOS_WAVE_BYTES / CHARPOS_CHUNK) + (lane >> 2);
        if ((lane & 3) == 0 && c < p.nchunks) {
            p.lead[c] = lead;
            if (p.four) p.four[c] = four;
            p.counts[c] = charpos_chunk_count(lead, four);
        }
    }
}

__global__ __launch_bounds__(256) void k_char_docs(CharposParams p)
{
    const CharIndex ix{p.lead, p.four, p.P};
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t d = (int64_t)blockIdx.x * 256 + threadIdx.x; d < p.ndocs; d += stride) {
        const CharDoc doc = charpos_doc(p.doc_off[d], p.doc_off[d + 1], p.total_bytes);
        if (doc.bad) atomicOr(p.status, BF_STATUS_BAD_OFFSETS);
        if (p.doc_units) p.doc_units[d] = charpos_units32(charpos_units(ix, doc));
    }
}

// the last q in [0, n) with off[q] <= t, by the 64 lanes of the calling wave together (wave-uniform; q = 0 where no entry is <= t)
__device__ __forceinline__ int64_t wave_find_doc(const int64_t *off, int64_t n, int64_t t)
{
    int64_t lo = 0, hi = n;
    const int lane = lane_id();
    while (hi - lo > 1) {
        const int64_t at = stream_probe(lo, hi, lane);
        const bool yes = at >= 0 && off[at] <= t;
        stream_narrow(&lo, &hi, __ballot(yes));
    }
    return lo;
}

template <int DIR>
__device__ __forceinline__ void char_items(const CharposParams &p)
{
    const CharIndex ix{p.lead, p.four, p.P};
    const int lane = lane_id();
    const int64_t all = p.item_off ? p.item_off[p.ndocs] : p.ndocs;
    const int64_t n = all < p.items_cap ? all : p.items_cap;
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i0 = (int64_t)blockIdx.x * 256 + (threadIdx.x & ~63u); i0 < n; i0 += stride) {       // i0 = the wave's first item: the bound is uniform
        const int64_t i = i0 + lane;
        int64_t d = i;
        bool held = true;
        if (p.item_off) {
            const int64_t last = i0 + 63 < n ? i0 + 63 : n - 1;
            const int64_t dlo = wave_find_doc(p.item_off, p.ndocs, i0), dhi = wave_find_doc(p.item_off, p.ndocs, last);
            const int64_t mine = i < last ? i : last;
            d = charpos_item_doc(p.item_off, dlo, dhi, mine);
            held = p.item_off[d] <= mine && mine < p.item_off[d + 1];      // (false only where the offsets do not start at 0 or decrease)
        }
        if (i >= n) continue;
        bool bad = !held;
        int32_t s = -1, e = -1;
        if (held) {
            const CharDoc doc = charpos_doc(p.doc_off[d], p.doc_off[d + 1], p.total_bytes);
            const int64_t Gb = doc.n > 0 ? charpos_G(ix, doc.b) : 0;
            const int64_t U = DIR == CHARPOS_INV ? charpos_units(ix, doc) : 0;
            if (p.starts) s = charpos_convert(ix, doc, Gb, U, DIR, p.flags, false, p.starts[i], &bad);
            if (p.ends) e = charpos_convert(ix, doc, Gb, U, DIR, p.flags, true, p.ends[i], &bad);
        }
        if (p.starts_out) p.starts_out[i] = s;
        if (p.ends_out) p.ends_out[i] = e;
        if (bad) atomicOr(p.status, BF_STATUS_BAD_OFFSETS);
    }
}

__global__ __launch_bounds__(256) void k_char_fwd(CharposParams p) { char_items<CHARPOS_FWD>(p); }
__global__ __launch_bounds__(256) void k_char_inv(CharposParams p) { char_items<CHARPOS_INV>(p); }

void launch_char_index(const CharposParams &p, hipStream_t s)
{
    const int64_t tiles = (p.total_bytes + CHARPOS_WAVE_BYTES - 1) / CHARPOS_WAVE_BYTES;
    if (tiles > 0) hipLaunchKernelGGL(k_char_index, dim3(rows_blocks(tiles * 64)), dim3(256), 0, s, p);
}

void launch_char_docs(const CharposParams &p, hipStream_t s)
{
    if (p.ndocs > 0) hipLaunchKernelGGL(k_char_docs, dim3(rows_blocks(p.ndocs)), dim3(256), 0, s, p);
}

// items_bound = what the host knows of the item count: items_cap, and ndocs where there are no item offsets
void launch_char_items(const CharposParams &p, int64_t items_bound, hipStream_t s)
{
    if (items_bound <= 0) return;
    if (p.dir == CHARPOS_FWD) hipLaunchKernelGGL(k_char_fwd, dim3(rows_blocks(items_bound)), dim3(256), 0, s, p);
    else hipLaunchKernelGGL(k_char_inv, dim3(rows_blocks(items_bound)), dim3(256), 0, s, p);
}

} // namespace bfa
