// k_ref_kmers: BwaIndex::get_kmers (bwa_index.hpp:247-255) for a batch of reference stretches = seq_to_kmers (bp.hpp:125-146) over the
// packed text, and for the minus strand kmers_revcomp (bp.hpp:82-99), straight out of the packed words in HBM.
//
// Every k-mer is a function of its own ten bits: no rolling state runs along a stretch and no pass reverses it.  A lane makes 16
// consecutive OUTPUTS: 16 five-mers overlap to 20 bases = 40 bits, which lie in at most three aligned 32-bit words of the text.  The
// text stores the first base of a byte in its top bits, so a byte-swapped word holds its 16 bases in bit order, and the 40 bits
// are one funnel shift.  Forward, output slot j is bits [39 - 2 j, 30 - 2 j] of them.  For the minus strand the lane reverse-complements
// the 40 bits once (complement, then the 2-bit groups mirrored): the reverse complement of the 5-mer at window base b is the 5-mer at
// base 15 - b of the mirrored window, so the slots again come out in output order.
//
// A run (refseq_dev.h) is one wavefront's work, a contiguous piece of one stretch: lane l takes the outputs [16 l - a, 16 l - a + 16)
// of the run (then those 1024 further on, for a run longer than the host cuts them), where a is what the run's first output lies past a
// 16-byte boundary, in elements.  So every 16 outputs that lie fully inside the run go out as two aligned 16-byte stores, a
// wavefront's stores are one contiguous 2 KB, and its loads are 256 contiguous bytes of the text; the ragged first and last
// outputs of a run are stored one by one.  The library starts every query's rows at a multiple of 8 elements (unc_refseq.cpp), which
// leaves only the last 16 outputs of a stretch ragged.  No LDS, no collectives.
#include <hip/hip_runtime.h>

#include "refseq_dev.h"

namespace unc {
namespace {

constexpr uint32_t RK_WAVES = 4;      // wavefronts (runs at a time) per workgroup

// the 20 bases from base (bit / 2) on, first base in bits 39-38
__device__ __forceinline__ uint64_t window40(const uint32_t *pac, uint64_t bit) {
    const uint32_t *w = pac + (bit >> 5);
    const uint32_t sh = (uint32_t)bit & 31u;          // even
    const uint64_t hi = ((uint64_t)__builtin_bswap32(w[0]) << 32) | (uint64_t)__builtin_bswap32(w[1]);
    uint64_t v = hi << sh;
    if (sh) v |= (uint64_t)__builtin_bswap32(w[2]) >> (32u - sh);
    return v >> 24;
}

// the reverse complement of a window of 20 bases
__device__ __forceinline__ uint64_t revcomp40(uint64_t v) {
    uint64_t x = ~v & 0xFFFFFFFFFFull;
    x = ((x >> 2) & 0x3333333333333333ull) | ((x & 0x3333333333333333ull) << 2);
    x = ((x >> 4) & 0x0F0F0F0F0F0F0F0Full) | ((x & 0x0F0F0F0F0F0F0F0Full) << 4);
    return __builtin_bswap64(x) >> 24;
}

__device__ __forceinline__ uint32_t slot(uint64_t v, uint32_t j) { return (uint32_t)(v >> (30u - 2u * j)) & 1023u; }

__global__ void __launch_bounds__(64 * RK_WAVES) k_ref_kmers(const uint32_t *pac, const RefKmerRun *runs, uint32_t n_runs, uint16_t *out) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (uint32_t r = blockIdx.x * RK_WAVES + wave; r < n_runs; r += gridDim.x * RK_WAVES) {
        const RefKmerRun R = runs[r];
        uint16_t *dst = out + R.out_off;
        const uint32_t a = (uint32_t)(((uintptr_t)dst >> 1) & 7u);
        // outputs [lo, hi) of the run, of the 16 that begin at `first` (below zero for the run's first piece when a > 0)
        for (int64_t first = (int64_t)lane * REF_KMERS_PER_LANE - a; first < (int64_t)R.n; first += 64 * REF_KMERS_PER_LANE) {
            const uint32_t lo = first < 0 ? 0u : (uint32_t)first;
            const uint32_t hi = (uint64_t)(first + REF_KMERS_PER_LANE) < R.n ? (uint32_t)(first + REF_KMERS_PER_LANE) : R.n;
            // forward: the window begins at output lo's base and slot j is output lo + j.  Minus strand: output o is the 5-mer at
            // base n - 1 - o, so the window begins at output (hi - 1)'s base and slot j of its mirror image is output hi - 16 + j
            uint64_t v;
            uint32_t s0;
            if (R.fwd) {
                v = window40(pac, R.pac_bit + 2ull * lo);
                s0 = 0;
            } else {
                v = revcomp40(window40(pac, R.pac_bit + 2ull * (R.n - hi)));
                s0 = REF_KMERS_PER_LANE - (hi - lo);
            }
            if (hi - lo == REF_KMERS_PER_LANE) {       // (first == lo: 16 bytes past the boundary a multiple of 32 bytes times)
                uint32_t p[8];
                for (uint32_t t = 0; t < 8; ++t) p[t] = slot(v, 2 * t) | (slot(v, 2 * t + 1) << 16);
                uint4 *d4 = (uint4 *)(dst + lo);
                d4[0] = make_uint4(p[0], p[1], p[2], p[3]);
                d4[1] = make_uint4(p[4], p[5], p[6], p[7]);
            } else {
                for (uint32_t o = lo; o < hi; ++o) dst[o] = (uint16_t)slot(v, s0 + (o - lo));
            }
        }
    }
}

}  // namespace

void launch_ref_kmers(const uint32_t *pac, const RefKmerRun *runs, uint32_t n_runs, uint16_t *out, uint32_t max_blocks, hipStream_t st) {
    if (n_runs == 0) return;
    uint32_t grid = (n_runs + RK_WAVES - 1) / RK_WAVES;
    if (max_blocks && grid > max_blocks) grid = max_blocks;
    hipLaunchKernelGGL(k_ref_kmers, dim3(grid), dim3(64 * RK_WAVES), 0, st, pac, runs, n_runs, out);
}

}  // namespace unc
