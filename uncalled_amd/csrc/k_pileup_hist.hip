// The pile-up's level histograms (pileup_dev.h): 64 buckets of 32 bits a bin around the bin's centre, the model's mean for the bin's
// k-mer in fixed point.
//
//   k_pileup_hist_accum     behind k_pileup_accum, over the same records with the same grid and the same two modes: a record that
//                           k_pileup_accum adds to a bin (not shared and skipped, not dropped, not outside: pileup_add's tests in
//                           their order) adds 1 to one bucket of that bin, one 32-bit atomic on global memory, device scope.  A
//                           kernel of its own, so that k_pileup_accum is the kernel it was: fused into it the add cost a pile-up
//                           WITHOUT a histogram 0.8 % when measured (profiles/pileup_hist_first_measurement.txt).
//   k_pileup_hist_centres   once, when the histogram is attached: a lane a position of the table.  It finds the position's region by
//                           a binary search over the first bins, takes the 20 bases from its base on out of the packed text with
//                           k_refseq.hip's window40 (the forward 5-mer is slot 0, its reverse complement slot 15 of the mirrored
//                           window) and writes the two strands' centres, looked up in a table of 1024, as one 16-byte store.
//   k_pileup_hist_gather, k_pileup_centres_gather   listed bins' rows and centres into dense buffers;  k_pileup_hist_merge  one
//                           histogram added into another, a lane a bucket, behind k_pileup_merge.
//   k_pileup_ks             the two-sample Kolmogorov-Smirnov distance of listed bins, exact: a wavefront a bin, a lane a bucket.  The two
//                           rows are two coalesced 256-byte loads; an inclusive prefix sum of each over the wavefront gives the
//                           cumulative counts A(k), B(k) and the totals n_a = A(63), n_b = B(63) (32 bits: the host refuses bins
//                           with n >= 2^32).  |A(k) / n_a - B(k) / n_b| = |A(k) n_b - B(k) n_a| / (n_a n_b): the numerator is a
//                           difference of two products below 2^64, its maximum over the lanes a butterfly of six steps, the lowest
//                           lane that has it a ballot.  No LDS: the four wavefronts of a workgroup take four bins.
#include <hip/hip_runtime.h>

#include <math.h>

#include "align_dev.h"
#include "dtw_dev.h"
#include "model_dev.h"
#include "pileup_dev.h"
#include "refseq_dev.h"
#include "wave_prims.h"

namespace unc {
namespace {

// one record into its bucket: pileup_add (k_pileup.hip) without the sums and the counters
__device__ inline void pileup_hist_add(const PileupAccum &A, const PileupHist &H, int32_t rid, uint64_t p, uint32_t fwd, float level, uint32_t shared) {
    if (shared && !(A.flags & UNC_PILEUP_KEEP_SHARED)) return;
    if ((__float_as_uint(level) & 0x7F800000u) == 0x7F800000u || !(fabsf(level) < MODEL_LEVEL_LIMIT)) return;
    uint64_t bin = 0;
    if (!pileup_bin(A, rid, p, fwd ? 0u : 1u, &bin)) return;
    UNC_SIM_CHECK(bin < A.n_bins);
    if (bin >= A.n_bins) return;                        // (cannot happen: the bins of the regions are the table's)
    const long long q = llrint((double)level * MODEL_Q_ONE);
    atomicAdd(H.hist + PILEUP_HIST_BUCKETS * bin + pileup_bucket(q, H.centres[bin], H.w), 1u);
}

// k_pileup_accum's two loops (the caller's arrays; a round's records behind k_align_segments), bound for bound
__global__ void __launch_bounds__(PILEUP_BLOCK) k_pileup_hist_accum(PileupAccum A, PileupHist H) {
    if (!A.jobs) {
        const uint64_t lo = (uint64_t)blockIdx.x * PILEUP_RECS_PER_BLOCK;
        const uint64_t hi = lo + PILEUP_RECS_PER_BLOCK < A.n ? lo + PILEUP_RECS_PER_BLOCK : A.n;
        for (uint64_t i = lo + threadIdx.x; i < hi; i += PILEUP_BLOCK)
            pileup_hist_add(A, H, A.rid[i], A.pos[i], A.fwd[i], A.level[i], A.shared ? A.shared[i] : 0u);
    } else {
        for (uint32_t a = blockIdx.x; a < A.n_jobs; a += gridDim.x) {
            const uint32_t q = A.jobs[a].out;
            const unc_seg_info_t inf = A.info[q];
            if (inf.status == UNC_SEG_NONE) continue;
            const AlignQuery Q = A.queries[q];
            const unc_ref_stretch_t T = A.stretches[q];
            const uint64_t room = A.seg_off[q + 1] - A.seg_off[q];
            uint32_t n = (uint64_t)inf.n_rows < room ? inf.n_rows : (uint32_t)room;
            if ((uint64_t)inf.row_first + n > Q.n_km) n = inf.row_first < Q.n_km ? Q.n_km - inf.row_first : 0;       // (cannot happen)
            const unc_segment_t *seg = A.seg + A.seg_off[q];
            for (uint32_t s = threadIdx.x; s < n; s += PILEUP_BLOCK) {
                const uint64_t row = (uint64_t)inf.row_first + s;
                const uint64_t p = T.fwd ? T.st + row : T.en - 5 - row;
                pileup_hist_add(A, H, T.rid, p, T.fwd, seg[s].level, seg[s].shared);
            }
        }
    }
}

__global__ void __launch_bounds__(PILEUP_BLOCK) k_pileup_hist_centres(const uint32_t *pac, const PileupRegion *regions, const uint64_t *base,
                                                                      uint32_t n_regions, uint64_t n_pos, const int64_t *ctab, int64_t *centres) {
    const uint64_t at = (uint64_t)blockIdx.x * PILEUP_BLOCK + threadIdx.x;
    if (at >= n_pos) return;
    // the region that holds position `at` of the table: the first one that ends behind it (unc_pileup.cpp: region_of_bin)
    uint32_t lo = 0, hi = n_regions;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (regions[mid].bin0 + regions[mid].n <= at) lo = mid + 1;
        else hi = mid;
    }
    UNC_SIM_CHECK(lo < n_regions && regions[lo].bin0 <= at);
    if (lo >= n_regions) return;                        // (cannot happen: the positions of the regions are the table's)
    const uint64_t g = base[lo] + (at - regions[lo].bin0);
    const uint64_t v = window40(pac, 2 * g);
    const uint32_t kf = slot(v, 0), kr = slot(revcomp40(v), REF_KMERS_PER_LANE - 1);
    *(ulonglong2 *)(centres + 2 * at) = make_ulonglong2((unsigned long long)ctab[kf], (unsigned long long)ctab[kr]);
}

__global__ void __launch_bounds__(PILEUP_BLOCK) k_pileup_hist_gather(const uint32_t *hist, const uint64_t *bins, uint64_t n, uint32_t *out) {
    const uint64_t i = (uint64_t)blockIdx.x * PILEUP_BLOCK + threadIdx.x;
    if (i >= n * PILEUP_HIST_BUCKETS) return;
    out[i] = hist[PILEUP_HIST_BUCKETS * bins[i / PILEUP_HIST_BUCKETS] + i % PILEUP_HIST_BUCKETS];
}

__global__ void __launch_bounds__(PILEUP_BLOCK) k_pileup_centres_gather(const int64_t *centres, const uint64_t *bins, uint64_t n, int64_t *out) {
    const uint64_t i = (uint64_t)blockIdx.x * PILEUP_BLOCK + threadIdx.x;
    if (i < n) out[i] = centres[bins[i]];
}

// nothing else touches either histogram meanwhile, so the adds are plain
__global__ void __launch_bounds__(PILEUP_BLOCK) k_pileup_hist_merge(uint32_t *dst, const uint32_t *src, uint64_t n_buckets) {
    const uint64_t i = (uint64_t)blockIdx.x * PILEUP_BLOCK + threadIdx.x;
    if (i < n_buckets) dst[i] += src[i];
}

constexpr uint32_t KS_WAVES = PILEUP_BLOCK / 64;

__global__ void __launch_bounds__(PILEUP_BLOCK) k_pileup_ks(const uint32_t *hist_a, const uint32_t *hist_b, const uint64_t *bins, uint64_t n,
                                                            PileupKs *out) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t i = (uint64_t)blockIdx.x * KS_WAVES + wave;
    if (i >= n) return;                                 // uniform over the wavefront
    const uint64_t row = PILEUP_HIST_BUCKETS * bins[i] + lane;
    const uint32_t a = hist_a[row], b = hist_b[row];
    uint32_t n_a = 0, n_b = 0;
    const uint32_t A = incl_sum32(a, &n_a), B = incl_sum32(b, &n_b);
    const uint64_t x = (uint64_t)A * n_b, y = (uint64_t)B * n_a;
    const uint64_t diff = x > y ? x - y : y - x;
    uint64_t num = diff;
#pragma unroll
    for (uint32_t d = 32; d > 0; d >>= 1) {
        const uint64_t o = xor_lane64(num, d);
        num = num > o ? num : o;
    }
    const uint32_t bucket = (uint32_t)__ffsll(__ballot(diff == num)) - 1u;        // some lane has the maximum
    const uint32_t s = bcast32(x > y ? 1u : x < y ? 2u : 0u, (int)bucket);
    if (lane == 0) {
        PileupKs o;
        o.n_a = n_a; o.n_b = n_b; o.num = num; o.bucket = bucket; o.sign = s == 1u ? 1 : s == 2u ? -1 : 0;
        out[i] = o;
    }
}

}  // namespace

// launch_pileup_accum's grid
void launch_pileup_hist_accum(const PileupAccum &a, const PileupHist &h, uint64_t n_records, hipStream_t st) {
    uint64_t grid = (n_records + PILEUP_RECS_PER_BLOCK - 1) / PILEUP_RECS_PER_BLOCK;
    if (a.jobs && grid > a.n_jobs) grid = a.n_jobs;
    if (grid == 0) return;
    hipLaunchKernelGGL(k_pileup_hist_accum, dim3((uint32_t)grid), dim3(PILEUP_BLOCK), 0, st, a, h);
}

void launch_pileup_hist_centres(const uint32_t *pac, const PileupRegion *regions, const uint64_t *base, uint32_t n_regions, uint64_t n_pos,
                                const int64_t *ctab, int64_t *centres, hipStream_t st) {
    const uint64_t grid = (n_pos + PILEUP_BLOCK - 1) / PILEUP_BLOCK;
    if (grid == 0) return;
    hipLaunchKernelGGL(k_pileup_hist_centres, dim3((uint32_t)grid), dim3(PILEUP_BLOCK), 0, st, pac, regions, base, n_regions, n_pos, ctab, centres);
}

void launch_pileup_hist_gather(const uint32_t *hist, const uint64_t *bins, uint64_t n, uint32_t *out, hipStream_t st) {
    const uint64_t grid = (n * PILEUP_HIST_BUCKETS + PILEUP_BLOCK - 1) / PILEUP_BLOCK;
    if (grid == 0) return;
    hipLaunchKernelGGL(k_pileup_hist_gather, dim3((uint32_t)grid), dim3(PILEUP_BLOCK), 0, st, hist, bins, n, out);
}

void launch_pileup_centres_gather(const int64_t *centres, const uint64_t *bins, uint64_t n, int64_t *out, hipStream_t st) {
    const uint64_t grid = (n + PILEUP_BLOCK - 1) / PILEUP_BLOCK;
    if (grid == 0) return;
    hipLaunchKernelGGL(k_pileup_centres_gather, dim3((uint32_t)grid), dim3(PILEUP_BLOCK), 0, st, centres, bins, n, out);
}

void launch_pileup_hist_merge(uint32_t *dst, const uint32_t *src, uint64_t n_bins, hipStream_t st) {
    const uint64_t n_buckets = n_bins * PILEUP_HIST_BUCKETS, grid = (n_buckets + PILEUP_BLOCK - 1) / PILEUP_BLOCK;
    if (grid == 0) return;
    hipLaunchKernelGGL(k_pileup_hist_merge, dim3((uint32_t)grid), dim3(PILEUP_BLOCK), 0, st, dst, src, n_buckets);
}

void launch_pileup_ks(const uint32_t *hist_a, const uint32_t *hist_b, const uint64_t *bins, uint64_t n, PileupKs *out, hipStream_t st) {
    const uint64_t grid = (n + KS_WAVES - 1) / KS_WAVES;
    if (grid == 0) return;
    hipLaunchKernelGGL(k_pileup_ks, dim3((uint32_t)grid), dim3(PILEUP_BLOCK), 0, st, hist_a, hist_b, bins, n, out);
}

}  // namespace unc
