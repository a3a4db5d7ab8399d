// bf_kernels_w2h.hip -- word hyphenation as a batch (bf_w2h.h has the lane programs and what they reproduce).
//
//  k_w2h_prep   lane per word: strict UTF-8 decode, BOM skip, the 300-character cut, class per position into the word's slot of the
//               position stream, characters and source bytes per word; words whose offsets leave the text are empty (status bit 3).
//  k_w2h_walk   lane per (word, From).  A workgroup takes W2H_WPB consecutive words, lays their positions side by side (a pass holds as
//               many whole words as fit W2H_PCAP positions: all 64 unless the words are long) and every lane walks from one position,
//               ORing `1 << value` into a byte per output slot in LDS.  Behind a barrier the bytes are resolved into "a hyphen follows"
//               flags (written over the word's classes), hyphens are counted per word, and the word's output size is stored.
//  (scan)       k_scan_* of bf_kernels_sp.hip over the sizes -> text offsets.
//  k_w2h_copy   lane per word: characters and hyphens to the scanned offset, never at or past the capacity.
#include "bf_kernels_common.h"
#include "bf_w2h.h"

namespace bfa {

constexpr int W2H_WPB = 64;               // words per workgroup round
constexpr int W2H_PCAP = 4096;            // positions per pass (one byte of LDS each); a word has at most 302

__global__ __launch_bounds__(256) void k_w2h_prep(W2hParams p)
{
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x; w < p.nwords; w += stride) {
        const int64_t b = p.word_off[w], e = p.word_off[w + 1];
        int nch = 0, srcb = 0;
        if (b < 0 || e < b || e > p.total_bytes) atomicOr(p.status, BF_STATUS_BAD_OFFSETS);
        else nch = w2h_prep_word(p.t, p.text + b, e - b, p.cls + w2h_slot(b, w), &srcb);
        p.nch[w] = nch; p.srcb[w] = srcb;
    }
}

__global__ __launch_bounds__(256) void k_w2h_walk(W2hParams p)
{
    __shared__ uint32_t s_seen[W2H_PCAP / 4];
    __shared__ int s_nch[W2H_WPB], s_lb[W2H_WPB + 1];
    __shared__ uint32_t s_nhy[W2H_WPB];
    const int tid = (int)threadIdx.x;
    const int64_t nrounds = (p.nwords + W2H_WPB - 1) / W2H_WPB;
    for (int64_t r = blockIdx.x; r < nrounds; r += gridDim.x) {
        const int64_t w0 = r * W2H_WPB;
        const int nw = (int)(p.nwords - w0 < W2H_WPB ? p.nwords - w0 : W2H_WPB);
        __syncthreads();                                           // the round before has read s_nch / s_nhy
        if (tid < W2H_WPB) {
            const int nch = tid < nw ? p.nch[w0 + tid] : 0;
            s_nch[tid] = nch; s_nhy[tid] = 0;
            const int inc = wave_incl_scan(nch > 0 ? nch + 2 : 0);   // (wave 0 is the first 64 threads)
            if (tid == 0) s_lb[0] = 0;
            s_lb[tid + 1] = inc;
        }
        __syncthreads();
        for (int wc = 0; wc < nw;) {
            int we = wc + 1;                                       // a pass: the words [wc, we), as many as fit
            while (we < nw && s_lb[we + 1] - s_lb[wc] <= W2H_PCAP) ++we;
            const int base = s_lb[wc], npos = s_lb[we] - base;
            for (int k = tid; k < (npos + 3) / 4; k += 256) s_seen[k] = 0;
            __syncthreads();
            for (int q = tid; q < npos; q += 256) {
                int lo = wc, hi = we - 1;                          // the word of position q: the last one that begins at or before it
                while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (s_lb[mid] - base <= q) lo = mid; else hi = mid - 1; }
                const int at = s_lb[lo] - base, from = q - at, nch = s_nch[lo];
                if (!w2h_starts_at(p.t, nch, from)) continue;
                const uint16_t *cls = p.cls + w2h_slot(p.word_off[w0 + lo], w0 + lo);
                w2h_walk(p.t, cls, nch, from, [&](int slot, int v) {
                    const int x = at + 1 + slot;                   // the slot's own position: 0 <= slot < nch
                    atomicOr(&s_seen[x >> 2], (1u << v) << (8 * (x & 3)));
                });
            }
            __syncthreads();
            for (int q = tid; q < npos; q += 256) {
                int lo = wc, hi = we - 1;
                while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (s_lb[mid] - base <= q) lo = mid; else hi = mid - 1; }
                const int i = q - (s_lb[lo] - base) - 1, nch = s_nch[lo];
                if (i < 0 || i >= nch) continue;                   // the anchors
                const bool hy = w2h_hyphen_after(p.t, (s_seen[q >> 2] >> (8 * (q & 3))) & 0xFFu, i, nch);
                p.cls[w2h_slot(p.word_off[w0 + lo], w0 + lo) + 1 + i] = hy ? 1 : 0;
                if (hy) atomicAdd(&s_nhy[lo], 1u);
            }
            __syncthreads();
            wc = we;
        }
        if (tid < nw) p.lens[w0 + tid] = s_nch[tid] > 0 ? p.srcb[w0 + tid] + (int)s_nhy[tid] * p.hy_len : 0;
    }
}

__global__ __launch_bounds__(256) void k_w2h_copy(W2hParams p)
{
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x; w < p.nwords; w += stride) {
        const int64_t o0 = p.out_off[w];
        const int nch = p.nch[w];
        if (nch <= 0 || p.out_off[w + 1] <= o0 || o0 >= p.out_cap) continue;
        const int64_t b = p.word_off[w], n = p.word_off[w + 1] - b;      // (nch > 0: the offsets are in range)
        const uint8_t *s = p.text + b;
        if (n >= 3 && s[0] == 0xEF && s[1] == 0xBB && s[2] == 0xBF) s += 3;
        w2h_copy_word(s, nch, p.cls + w2h_slot(b, w) + 1, p.hy_bytes, p.hy_len, [&](int o, uint8_t c) {
            if (o0 + o < p.out_cap) p.out[o0 + o] = c;
        });
    }
}

static unsigned w2h_blocks(int64_t items, int per_block, int per_cu)
{
    int64_t blocks = (items + per_block - 1) / per_block;
    if (blocks > (int64_t)device_cus() * per_cu) blocks = (int64_t)device_cus() * per_cu;
    return (unsigned)(blocks < 1 ? 1 : blocks);
}

void launch_w2h_prep(const W2hParams &p, hipStream_t s) { hipLaunchKernelGGL(k_w2h_prep, dim3(w2h_blocks(p.nwords, 256, 32)), dim3(256), 0, s, p); }
void launch_w2h_walk(const W2hParams &p, hipStream_t s) { hipLaunchKernelGGL(k_w2h_walk, dim3(w2h_blocks(p.nwords, W2H_WPB, 32)), dim3(256), 0, s, p); }
void launch_w2h_copy(const W2hParams &p, hipStream_t s) { hipLaunchKernelGGL(k_w2h_copy, dim3(w2h_blocks(p.nwords, 256, 32)), dim3(256), 0, s, p); }

} // namespace bfa
