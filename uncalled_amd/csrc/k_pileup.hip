// The signal pile-up at reference coordinates: the records of k_align_segments (k_segments.hip), summed per bin = (position of the
// k-mer's leftmost forward base, strand) over many reads, and the kernels that find and read the covered bins of the table.
//
//   k_pileup_accum   per record: n += 1, S += q, SS += q * q (128 bits, two words), D += smp_n, q = llrint((double)level * 2^20) as in
//                    k_model.hip, with its limits and its carry rule: the atomic on the low word returns the value it found,
//                    old + x < old says the low word wrapped, and then 1 goes to the high word.  All integers: the table does not
//                    depend on the order of the records or on how they are cut into launches.  A position has no small key space,
//                    so there is no table in LDS: every add is a 64-bit atomic on global memory, device scope, the operations of
//                    k_model_accum's flush.  A bin's five words are adjacent (pileup_dev.h): a record's atomics fall into one or two
//                    cache lines.  The region of a position is found per record by a binary search over the sorted region table.
//   k_pileup_count, k_pileup_scan, k_pileup_write
//                    the indices of the covered bins in ascending order, as an ordered compaction in three launches: per-workgroup
//                    counts (ballot and popcount over the wavefront), an exclusive scan of the counts by one workgroup, the write.
//                    No workgroup waits for another.
//   k_pileup_gather  the five words of listed bins into a dense buffer;  k_pileup_merge  one table added into another.
#include <hip/hip_runtime.h>

#include <math.h>

#include "align_dev.h"
#include "dtw_dev.h"
#include "model_dev.h"
#include "pileup_dev.h"
#include "wave_prims.h"

namespace unc {
namespace {

// the region that holds position p of sequence rid: the last one with (rid, st) <= (rid, p), if p lies inside it
__device__ inline bool pileup_bin(const PileupAccum &A, int32_t rid, uint64_t p, uint32_t strand, uint64_t *bin) {
    uint32_t lo = 0, hi = A.n_regions;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        const int32_t r = A.regions[mid].rid;
        if (r < rid || (r == rid && A.regions[mid].st <= p)) lo = mid + 1;
        else hi = mid;
    }
    if (lo == 0) return false;
    const PileupRegion R = A.regions[lo - 1];
    if (R.rid != rid || p - R.st >= R.n) return false;
    *bin = 2 * (R.bin0 + (p - R.st)) + strand;
    return true;
}

// one record into the table; cnt: this lane's counters (PILEUP_DROPPED, _OUTSIDE, _ADDED)
__device__ inline void pileup_add(const PileupAccum &A, int32_t rid, uint64_t p, uint32_t fwd, float level, uint32_t smp_n, uint32_t shared,
                                  uint64_t *cnt) {
    if (shared && !(A.flags & UNC_PILEUP_KEEP_SHARED)) return;
    // not finite, or |level| >= 2048 (a NaN compares false: the exponent test comes first)
    if ((__float_as_uint(level) & 0x7F800000u) == 0x7F800000u || !(fabsf(level) < MODEL_LEVEL_LIMIT)) { ++cnt[PILEUP_DROPPED]; return; }
    uint64_t bin = 0;
    if (!pileup_bin(A, rid, p, fwd ? 0u : 1u, &bin)) { ++cnt[PILEUP_OUTSIDE]; return; }
    UNC_SIM_CHECK(bin < A.n_bins);
    if (bin >= A.n_bins) return;                        // (cannot happen: the bins of the regions are the table's)
    const double scaled = (double)level * MODEL_Q_ONE;  // exact: a float times a power of two
    const long long q = llrint(scaled);                 // round to nearest even
    const unsigned long long qq = (unsigned long long)(q * q);
    unsigned long long *w = A.tab + PILEUP_WORDS * bin;
    atomicAdd(w + PILEUP_N, 1ull);
    atomicAdd(w + PILEUP_S, (unsigned long long)q);     // two's complement: the sum of the words is the word of the sum
    const unsigned long long old = atomicAdd(w + PILEUP_LO, qq);
    if (old + qq < old) atomicAdd(w + PILEUP_HI, 1ull);
    atomicAdd(w + PILEUP_D, (unsigned long long)smp_n);
    ++cnt[PILEUP_ADDED];
}

// One launch: the caller's arrays (A.jobs == null: workgroup b takes records [b, b + 1) * PILEUP_RECS_PER_BLOCK), or a round's records
// where k_align_segments left them (workgroup b takes every gridDim.x-th alignment of the round; record s of query q is row
// row_first + s of the query's stretch: position st + row on the plus strand, en - 5 - row on the minus strand, whose rows are the
// forward k-mers in reverse order, each reverse-complemented).  The choice is uniform over the grid
__global__ void __launch_bounds__(PILEUP_BLOCK) k_pileup_accum(PileupAccum A) {
    __shared__ unsigned long long tot[PILEUP_COUNTERS];
    if (threadIdx.x < PILEUP_COUNTERS) tot[threadIdx.x] = 0;
    __syncthreads();
    uint64_t cnt[PILEUP_COUNTERS] = {0, 0, 0};
    if (!A.jobs) {
        const uint64_t lo = (uint64_t)blockIdx.x * PILEUP_RECS_PER_BLOCK;
        const uint64_t hi = lo + PILEUP_RECS_PER_BLOCK < A.n ? lo + PILEUP_RECS_PER_BLOCK : A.n;
        for (uint64_t i = lo + threadIdx.x; i < hi; i += PILEUP_BLOCK)
            pileup_add(A, A.rid[i], A.pos[i], A.fwd[i], A.level[i], A.smp_n[i], A.shared ? A.shared[i] : 0u, cnt);
    } else {
        for (uint32_t a = blockIdx.x; a < A.n_jobs; a += gridDim.x) {
            const uint32_t q = A.jobs[a].out;
            const unc_seg_info_t inf = A.info[q];
            if (inf.status == UNC_SEG_NONE) continue;
            const AlignQuery Q = A.queries[q];
            const unc_ref_stretch_t T = A.stretches[q];
            const uint64_t room = A.seg_off[q + 1] - A.seg_off[q];
            UNC_SIM_CHECK((uint64_t)inf.n_rows <= room && (uint64_t)inf.row_first + inf.n_rows <= Q.n_km && T.en - T.st == (uint64_t)Q.n_km + 4);
            uint32_t n = (uint64_t)inf.n_rows < room ? inf.n_rows : (uint32_t)room;
            if ((uint64_t)inf.row_first + n > Q.n_km) n = inf.row_first < Q.n_km ? Q.n_km - inf.row_first : 0;       // (cannot happen)
            const unc_segment_t *seg = A.seg + A.seg_off[q];
            for (uint32_t s = threadIdx.x; s < n; s += PILEUP_BLOCK) {
                const uint64_t row = (uint64_t)inf.row_first + s;
                const uint64_t p = T.fwd ? T.st + row : T.en - 5 - row;
                pileup_add(A, T.rid, p, T.fwd, seg[s].level, seg[s].smp_n, seg[s].shared, cnt);
            }
        }
    }
    for (uint32_t c = 0; c < PILEUP_COUNTERS; ++c)
        if (cnt[c]) atomicAdd(&tot[c], (unsigned long long)cnt[c]);
    __syncthreads();
    if (threadIdx.x < PILEUP_COUNTERS && tot[threadIdx.x]) atomicAdd(A.tab + PILEUP_WORDS * A.n_bins + threadIdx.x, tot[threadIdx.x]);
}

// ---- the covered bins.  Workgroup g takes the bins [g, g + 1) * PILEUP_SCAN_CHUNK, its wavefront w the 256 from 256 w on, 64 a step
__device__ inline bool covered(const unsigned long long *a, const unsigned long long *b, uint64_t n_bins, uint64_t min_cov, uint64_t bin) {
    if (bin >= n_bins) return false;
    if (a[PILEUP_WORDS * bin + PILEUP_N] < min_cov) return false;
    return !b || b[PILEUP_WORDS * bin + PILEUP_N] >= min_cov;
}

constexpr uint32_t SCAN_WAVES = PILEUP_BLOCK / 64, SCAN_STEPS = PILEUP_SCAN_CHUNK / PILEUP_BLOCK;

__global__ void __launch_bounds__(PILEUP_BLOCK) k_pileup_count(const unsigned long long *a, const unsigned long long *b, uint64_t n_bins,
                                                               uint64_t min_cov, uint32_t *counts) {
    __shared__ uint32_t wsum[SCAN_WAVES];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t first = (uint64_t)blockIdx.x * PILEUP_SCAN_CHUNK + (uint64_t)wave * (64u * SCAN_STEPS);
    uint32_t n = 0;
    for (uint32_t s = 0; s < SCAN_STEPS; ++s) n += (uint32_t)__popcll(__ballot(covered(a, b, n_bins, min_cov, first + 64u * s + lane)));
    if (lane == 0) wsum[wave] = n;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0;
        for (uint32_t w = 0; w < SCAN_WAVES; ++w) t += wsum[w];
        counts[blockIdx.x] = t;
    }
}

// one workgroup: offsets[g] = the sum of counts[0 .. g), offsets[n_blocks] = the total.  A count is at most PILEUP_SCAN_CHUNK, so a
// wavefront's sum fits 32 bits; the running total is 64 bits wide
__global__ void __launch_bounds__(PILEUP_BLOCK) k_pileup_scan(const uint32_t *counts, uint64_t n_blocks, uint64_t *offsets) {
    __shared__ uint32_t wtot[SCAN_WAVES];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint64_t carry = 0;
    for (uint64_t base = 0; base < n_blocks; base += PILEUP_BLOCK) {
        const uint64_t i = base + threadIdx.x;
        const uint32_t v = i < n_blocks ? counts[i] : 0u;
        uint32_t tot = 0;
        const uint32_t pre = excl_sum32(v, &tot);
        if (lane == 0) wtot[wave] = tot;
        __syncthreads();
        uint32_t before = 0, all = 0;
        for (uint32_t w = 0; w < SCAN_WAVES; ++w) {
            if (w < wave) before += wtot[w];
            all += wtot[w];
        }
        if (i < n_blocks) offsets[i] = carry + before + pre;
        carry += all;
        __syncthreads();
    }
    if (threadIdx.x == 0) offsets[n_blocks] = carry;
}

__global__ void __launch_bounds__(PILEUP_BLOCK) k_pileup_write(const unsigned long long *a, const unsigned long long *b, uint64_t n_bins,
                                                               uint64_t min_cov, const uint64_t *offsets, uint64_t *out, uint64_t cap) {
    __shared__ uint32_t wsum[SCAN_WAVES];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t first = (uint64_t)blockIdx.x * PILEUP_SCAN_CHUNK + (uint64_t)wave * (64u * SCAN_STEPS);
    uint64_t mask[SCAN_STEPS];
    uint32_t n = 0;
    for (uint32_t s = 0; s < SCAN_STEPS; ++s) {
        mask[s] = __ballot(covered(a, b, n_bins, min_cov, first + 64u * s + lane));
        n += (uint32_t)__popcll(mask[s]);
    }
    if (lane == 0) wsum[wave] = n;
    __syncthreads();
    uint64_t at = offsets[blockIdx.x];
    for (uint32_t w = 0; w < wave; ++w) at += wsum[w];
    UNC_SIM_CHECK(at + n <= offsets[gridDim.x]);
    for (uint32_t s = 0; s < SCAN_STEPS; ++s) {
        const uint64_t idx = at + prefix_popc(mask[s]);
        if (((mask[s] >> lane) & 1ull) && idx < cap) out[idx] = first + 64u * s + lane;
        at += (uint32_t)__popcll(mask[s]);
    }
}

__global__ void __launch_bounds__(PILEUP_BLOCK) k_pileup_gather(const unsigned long long *tab, const uint64_t *bins, uint64_t n, unsigned long long *out) {
    const uint64_t i = (uint64_t)blockIdx.x * PILEUP_BLOCK + threadIdx.x;
    if (i >= n * PILEUP_WORDS) return;
    out[i] = tab[PILEUP_WORDS * bins[i / PILEUP_WORDS] + i % PILEUP_WORDS];
}

// one lane a bin; nothing else touches either table meanwhile, so the adds are plain.  The first lanes of the grid add the counters
__global__ void __launch_bounds__(PILEUP_BLOCK) k_pileup_merge(unsigned long long *dst, const unsigned long long *src, uint64_t n_bins) {
    const uint64_t i = (uint64_t)blockIdx.x * PILEUP_BLOCK + threadIdx.x;
    if (i < PILEUP_COUNTERS) dst[PILEUP_WORDS * n_bins + i] += src[PILEUP_WORDS * n_bins + i];
    if (i >= n_bins) return;
    unsigned long long *d = dst + PILEUP_WORDS * i;
    const unsigned long long *s = src + PILEUP_WORDS * i;
    if (s[PILEUP_N] == 0) return;
    d[PILEUP_N] += s[PILEUP_N];
    d[PILEUP_S] += s[PILEUP_S];
    const unsigned long long old = d[PILEUP_LO], lo = old + s[PILEUP_LO];
    d[PILEUP_LO] = lo;
    d[PILEUP_HI] += s[PILEUP_HI] + (lo < old ? 1ull : 0ull);
    d[PILEUP_D] += s[PILEUP_D];
}

}  // namespace

// the grid goes by the record count: a workgroup for every PILEUP_RECS_PER_BLOCK records (of a round: at most one per alignment)
void launch_pileup_accum(const PileupAccum &a, uint64_t n_records, hipStream_t st) {
    uint64_t grid = (n_records + PILEUP_RECS_PER_BLOCK - 1) / PILEUP_RECS_PER_BLOCK;
    if (a.jobs && grid > a.n_jobs) grid = a.n_jobs;
    if (grid == 0) return;
    hipLaunchKernelGGL(k_pileup_accum, dim3((uint32_t)grid), dim3(PILEUP_BLOCK), 0, st, a);
}

void launch_pileup_count(const unsigned long long *a, const unsigned long long *b, uint64_t n_bins, uint64_t min_cov, uint32_t *counts, hipStream_t st) {
    hipLaunchKernelGGL(k_pileup_count, dim3((uint32_t)pileup_scan_blocks(n_bins)), dim3(PILEUP_BLOCK), 0, st, a, b, n_bins, min_cov, counts);
}

void launch_pileup_scan(const uint32_t *counts, uint64_t n_blocks, uint64_t *offsets, hipStream_t st) {
    hipLaunchKernelGGL(k_pileup_scan, dim3(1), dim3(PILEUP_BLOCK), 0, st, counts, n_blocks, offsets);
}

void launch_pileup_write(const unsigned long long *a, const unsigned long long *b, uint64_t n_bins, uint64_t min_cov, const uint64_t *offsets,
                         uint64_t *out, uint64_t cap, hipStream_t st) {
    hipLaunchKernelGGL(k_pileup_write, dim3((uint32_t)pileup_scan_blocks(n_bins)), dim3(PILEUP_BLOCK), 0, st, a, b, n_bins, min_cov, offsets, out, cap);
}

void launch_pileup_gather(const unsigned long long *tab, const uint64_t *bins, uint64_t n, unsigned long long *out, hipStream_t st) {
    const uint64_t grid = (n * PILEUP_WORDS + PILEUP_BLOCK - 1) / PILEUP_BLOCK;
    if (grid == 0) return;
    hipLaunchKernelGGL(k_pileup_gather, dim3((uint32_t)grid), dim3(PILEUP_BLOCK), 0, st, tab, bins, n, out);
}

void launch_pileup_merge(unsigned long long *dst, const unsigned long long *src, uint64_t n_bins, hipStream_t st) {
    const uint64_t grid = n_bins ? (n_bins + PILEUP_BLOCK - 1) / PILEUP_BLOCK : 1;
    hipLaunchKernelGGL(k_pileup_merge, dim3((uint32_t)grid), dim3(PILEUP_BLOCK), 0, st, dst, src, n_bins);
}

}  // namespace unc
