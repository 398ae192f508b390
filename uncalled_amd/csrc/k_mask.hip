// Repeat masking on the device (include/uncalled_hip.h: unc_mask_*): the k-mer counting and masking loop of the reference's
// masking/mask_internal.sh + mask_kmers.py, and the window look-ups of masking/mask_external.sh through the FM index that is on
// the device anyway.  Integer work only: every result is exact and independent of the order the atomics arrive in.
// The layout of the text and of the flag bitmap is described in mask_dev.h.
#include <hip/hip_runtime.h>

#include "fm_dev.h"
#include "mask_dev.h"
#include "unc_dev_types.h"
#include "wave_prims.h"

namespace unc {

namespace {

__device__ __forceinline__ uint64_t global_tid() { return (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; }
__device__ __forceinline__ uint64_t global_threads() { return (uint64_t)gridDim.x * blockDim.x; }

// The windows of k bases that start in chunk c = positions [16 c, 16 c + 16): the lane reads the chunk's quad and the next one
// (k - 1 <= 12 bases behind the last start) and rolls the k-mer code (first base most significant, bp.hpp) and the length of the
// run of bases that may share a window over them.  emit(j, code): the window starting at 16 c + j exists and holds `code`.
// Windows that start before the chunk are the previous lane's: the run starts at 0 here.
template <class Emit> __device__ __forceinline__ void scan_chunk(const uint8_t *text, uint64_t c, uint32_t k, Emit emit) {
    const uint4 *q = reinterpret_cast<const uint4 *>(text) + c;
    const uint4 a = q[0], b = q[1];
    const uint32_t w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    const uint32_t kmask = (1u << (2u * k)) - 1u;      // k <= 13
    uint32_t run = 0, code = 0;
#pragma unroll
    for (uint32_t j = 0; j < MASK_RUN + MASK_MAX_K - 1; ++j) {
        if (j < MASK_RUN - 1 + k) {
            const uint32_t byte = (w[j >> 2] >> ((j & 3u) * 8u)) & 0xFFu;
            if (byte & MASK_CTG_START) run = 0;
            run = (byte & 7u) < 4u ? run + 1u : 0u;
            code = ((code << 2) | (byte & 3u)) & kmask;
            if (run >= k) emit(j + 1u - k, code);
        }
    }
}

}  // namespace

// Counts every window of k bases (jellyfish count -m k without -C, mask_internal.sh:47) into 4^k counters: one chunk per lane and
// trip, one integer atomic per window.  (A variant that collapsed equal neighbouring k-mers of a lane and of neighbouring lanes before
// the atomic was built and measured on the chr20-sized synthetic reference: 1.762 ms a pass against 1.739 ms for this one,
// profiles/mask_first_measurement.txt.  The faster one was kept.)
__global__ __launch_bounds__(MASK_BLOCK) void k_kmer_count(const uint8_t *text, uint64_t n, uint32_t k, uint32_t *counts, const MaskCtl *ctl) {
    if (ctl && ctl->stop) return;
    const uint64_t n_chunks = (n + MASK_RUN - 1) / MASK_RUN, stride = global_threads();
    for (uint64_t c = global_tid(); c < n_chunks; c += stride)
        scan_chunk(text, c, k, [&](uint32_t, uint32_t code) { atomicAdd(counts + code, 1u); });
}

// The largest count and the smallest k-mer code that has it, as the maximum of count << 32 | ~code: whatever order the
// wavefronts arrive in, the maximum is the same.
__global__ __launch_bounds__(MASK_BLOCK) void k_kmer_argmax(const uint32_t *counts, uint64_t n_kmers, MaskIter *it, const MaskCtl *ctl) {
    if (ctl && ctl->stop) return;
    const uint4 *q = reinterpret_cast<const uint4 *>(counts);
    const uint64_t n_quads = n_kmers >> 2, stride = global_threads();
    unsigned long long best = 0;
    for (uint64_t i = global_tid(); i < n_quads; i += stride) {
        const uint4 v = q[i];
        const uint32_t c4[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
            const unsigned long long key = ((unsigned long long)c4[j] << 32) | (0xFFFFFFFFu - (uint32_t)(4 * i + j));
            best = key > best ? key : best;
        }
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const unsigned long long o = xor_lane64(best, (uint32_t)d);
        best = o > best ? o : best;
    }
    if (lane_id() == 0 && best) atomicMax(&it->best, best);
}

// Flags the starts of the occurrences of the iteration's k-mer in the text as it stands (mask_kmers.py:16-27 finds overlapping
// occurrences, `find(kmer, i + 1)`: every start counts), and counts them ("masked %d occurences", mask_kmers.py:78).  Nothing is
// masked here: k_mask_cover runs after every start is known.  Every 16-bit word of the bitmap is written, set bits or not.
__global__ __launch_bounds__(MASK_BLOCK) void k_mask_flag_kmer(const uint8_t *text, uint64_t n, uint32_t k, MaskIter *it, const MaskCtl *ctl,
                                                              uint64_t *flags) {
    if (ctl->stop) return;
    const unsigned long long best = it->best;
    if ((best >> 32) < 2) return;                       // the loop ends here: k_mask_cover raises the stop flag
    const uint32_t target = 0xFFFFFFFFu - (uint32_t)best;
    uint16_t *f16 = reinterpret_cast<uint16_t *>(flags);
    const uint64_t n_chunks = 4 * ((n + 63) / 64), stride = global_threads();
    uint64_t occ = 0;
    for (uint64_t c = global_tid(); c < n_chunks; c += stride) {
        uint32_t bits = 0;
        scan_chunk(text, c, k, [&](uint32_t j, uint32_t code) { bits |= (code == target ? 1u : 0u) << j; });
        f16[c] = (uint16_t)bits;
        occ += (uint32_t)__popc(bits);
    }
    occ = wave_sum64(occ);
    if (lane_id() == 0 && occ) atomicAdd(&it->occ, (uint32_t)occ);
}

// Position p becomes code 4 iff a flagged start lies in [p - len + 1, p]; the bases that were not 4 before are counted.  One lane
// per 64 positions = one word of the bitmap and four quads of the text: it looks back for the last flagged start within reach,
// then rolls forward.  Shared by both modes (len = k or min_len).  `it` given: the internal loop, which ends here when the
// iteration's largest count is below 2 (nothing was flagged).
__global__ __launch_bounds__(MASK_BLOCK) void k_mask_cover(uint8_t *text, uint64_t n, uint32_t len, const uint64_t *flags, MaskIter *it,
                                                          MaskCtl *ctl, unsigned long long *bases64) {
    if (it) {
        if (ctl->stop) return;
        if ((it->best >> 32) < 2) {
            if (global_tid() == 0) ctl->stop = 1u;
            return;
        }
    }
    const uint64_t n_words = (n + 63) / 64, stride = global_threads();
    uint64_t newly = 0;
    for (uint64_t w = global_tid(); w < n_words; w += stride) {
        const uint64_t F = flags[w], p0 = w << 6;
        const uint64_t NONE = ~0ull;
        uint64_t last = NONE;
        const uint64_t lo = p0 >= (uint64_t)(len - 1u) ? p0 - (len - 1u) : 0;       // the earliest start that reaches into this word
        for (uint64_t v = w; v > 0 && ((v - 1) << 6) + 63 >= lo;) {
            --v;
            const uint64_t G = flags[v];
            if (G) { last = (v << 6) + 63u - (uint64_t)__clzll((long long)G); break; }
        }
        if (!F && (last == NONE || p0 - last >= len)) continue;
        uint4 *q = reinterpret_cast<uint4 *>(text + p0);
        uint4 t4[4] = {q[0], q[1], q[2], q[3]};
        uint32_t t[16] = {t4[0].x, t4[0].y, t4[0].z, t4[0].w, t4[1].x, t4[1].y, t4[1].z, t4[1].w,
                          t4[2].x, t4[2].y, t4[2].z, t4[2].w, t4[3].x, t4[3].y, t4[3].z, t4[3].w};
        uint32_t changed = 0;
#pragma unroll
        for (uint32_t j = 0; j < 64; ++j) {
            const uint64_t p = p0 + j;
            if ((F >> j) & 1ull) last = p;
            const bool covered = last != NONE && p - last < len;
            const uint32_t sh = (j & 3u) * 8u, byte = (t[j >> 2] >> sh) & 0xFFu;
            if (covered && (byte & 7u) < 4u) {
                t[j >> 2] = (t[j >> 2] & ~(0xFFu << sh)) | (((byte & MASK_CTG_START) | 4u) << sh);
                ++changed;
            }
        }
        if (changed) {
            UNC_SIM_CHECK(p0 + 64 <= ((n + 63) / 64) * 64);
            q[0] = make_uint4(t[0], t[1], t[2], t[3]); q[1] = make_uint4(t[4], t[5], t[6], t[7]);
            q[2] = make_uint4(t[8], t[9], t[10], t[11]); q[3] = make_uint4(t[12], t[13], t[14], t[15]);
            newly += changed;
        }
    }
    newly = wave_sum64(newly);
    if (lane_id() == 0 && newly) {
        if (it) atomicAdd(&it->bases, (uint32_t)newly);
        else atomicAdd(bases64, (unsigned long long)newly);
    }
}

// mask_external.sh:61-70: for every window of `len` bases of the target, the number of its occurrences in the index's text (both
// strands: bowtie -v 0) = the size of its SA interval, by backward search from the window's last base to its first.  One lane per
// window start, 64 consecutive starts per wavefront and trip, whose verdicts (count > min_copy, mask_external.sh:77) are one word
// of the bitmap.  A window that touches a code >= 4 or a contig's end does not exist (count 0).  Without the tap a lane stops as
// soon as its interval holds no more than min_copy rows -- intervals only shrink; with the tap every walk runs until the interval
// is empty or the window's first base is done, and the count is exact.
// FM32: the 32-bit rank table of a reference of fewer than 2^32 rows, else the BWA-format arithmetic in 64 bits.
template <bool FM32>
__global__ __launch_bounds__(MASK_BLOCK) void k_fm_window_count(DevIndex ix, const uint8_t *text, uint64_t n, uint32_t len, uint64_t min_copy,
                                                               uint64_t *flags, uint64_t *counts) {
    const uint64_t n_words = (n + 63) / 64, n_waves = global_threads() >> 6;
    const uint32_t lane = (uint32_t)lane_id();
    for (uint64_t w = global_tid() >> 6; w < n_words; w += n_waves) {
        const uint64_t p = (w << 6) + lane;
        uint64_t cnt = 0;
        bool exists = p + len <= n;
        for (uint32_t i = 0; exists && i < len; ++i) {               // (the text first: sequential bytes, against `len` scattered blocks)
            const uint32_t byte = text[p + i];
            if ((byte & 7u) >= 4u || (i > 0 && (byte & MASK_CTG_START))) exists = false;
        }
        if (exists) {
            uint32_t c = text[p + len - 1] & 3u;
            uint64_t s = fm_L2(ix, c) + 1, e = fm_L2(ix, c + 1u);       // the rows of the suffixes that start with c
            bool live = s <= e && (counts || e - s + 1 > min_copy);
            for (uint32_t i = 1; live && i < len; ++i) {
                c = text[p + len - 1 - i] & 3u;
                if (FM32) {
                    uint32_t s32, e32;
                    fm32_get_neighbor(ix, (uint32_t)s, (uint32_t)e, c, &s32, &e32);
                    s = s32; e = e32;
                } else fm_get_neighbor(ix, s, e, c, &s, &e);
                live = s <= e && (counts || e - s + 1 > min_copy);
            }
            if (live) cnt = e - s + 1;
        }
        if (counts && p < n) counts[p] = cnt;
        const uint64_t m = __ballot(cnt > min_copy);
        if (lane == 0) flags[w] = m;
    }
}

static inline uint32_t grid_for(uint64_t items, uint32_t blocks) {
    const uint64_t need = (items + MASK_BLOCK - 1) / MASK_BLOCK;
    return (uint32_t)(need < 1 ? 1 : (need < blocks ? need : blocks));
}

void launch_kmer_count(const uint8_t *text, uint64_t n, uint32_t k, uint32_t *counts, const MaskCtl *ctl, uint32_t blocks, hipStream_t st) {
    const uint32_t g = grid_for((n + MASK_RUN - 1) / MASK_RUN, blocks);
    hipLaunchKernelGGL(k_kmer_count, dim3(g), dim3(MASK_BLOCK), 0, st, text, n, k, counts, ctl);
}
void launch_kmer_argmax(const uint32_t *counts, uint64_t n_kmers, MaskIter *it, const MaskCtl *ctl, uint32_t blocks, hipStream_t st) {
    hipLaunchKernelGGL(k_kmer_argmax, dim3(grid_for(n_kmers >> 2, blocks)), dim3(MASK_BLOCK), 0, st, counts, n_kmers, it, ctl);
}
void launch_mask_flag_kmer(const uint8_t *text, uint64_t n, uint32_t k, MaskIter *it, const MaskCtl *ctl, uint64_t *flags, uint32_t blocks,
                           hipStream_t st) {
    hipLaunchKernelGGL(k_mask_flag_kmer, dim3(grid_for(4 * ((n + 63) / 64), blocks)), dim3(MASK_BLOCK), 0, st, text, n, k, it, ctl, flags);
}
void launch_mask_cover(uint8_t *text, uint64_t n, uint32_t len, const uint64_t *flags, MaskIter *it, MaskCtl *ctl,
                       unsigned long long *bases64, uint32_t blocks, hipStream_t st) {
    hipLaunchKernelGGL(k_mask_cover, dim3(grid_for((n + 63) / 64, blocks)), dim3(MASK_BLOCK), 0, st, text, n, len, flags, it, ctl, bases64);
}
void launch_fm_window_count(const DevIndex &ix, const uint8_t *text, uint64_t n, uint32_t len, uint64_t min_copy, uint64_t *flags,
                            uint64_t *counts, uint32_t blocks, hipStream_t st) {
    const uint32_t g = grid_for(((n + 63) / 64) * 64, blocks);
    if (ix.fm32) hipLaunchKernelGGL(k_fm_window_count<true>, dim3(g), dim3(MASK_BLOCK), 0, st, ix, text, n, len, min_copy, flags, counts);
    else hipLaunchKernelGGL(k_fm_window_count<false>, dim3(g), dim3(MASK_BLOCK), 0, st, ix, text, n, len, min_copy, flags, counts);
}

}  // namespace unc
