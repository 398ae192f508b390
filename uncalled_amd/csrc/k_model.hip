// k_model_accum: the training reduction of a pore model -- per k-mer, the count n, the sum S of q and the sum SS of q * q over the
// records of a batch, q = llrint((double)level * 2^20).  A pore model is the per-k-mer mean and deviation of the normalised levels
// of many alignments (the counterpart of PoreModel's file, pore_model.hpp:108-160); the records are k_align_segments' (k_segments.hip),
// read where they lie on the device, or the caller's arrays (unc_model_acc_add).
//
// Fixed point, not floating point: the conversion is deterministic and integer sums do not depend on their order, so the result is
// the same however the batch is cut into rounds, blocks and lanes.  |level| < 2048 (anything else is dropped and counted), so
// |q| < 2^31 and q * q < 2^62 fits one word; SS is kept in 128 bits as two words.
//
// A workgroup keeps a private table of the 1024 bins in LDS (n u32, S i64, SS low and high word: 28 KB of the CU's 160 KB), adds its
// records there with LDS atomics, and flushes the bins that are not empty to the accumulator in global memory with 64-bit atomics:
// at most four per bin and workgroup, instead of four per record.  The 128-bit add: the atomic on the low word returns the value it
// found; old + x < old says the low word wrapped, and then 1 goes to the high word.  Every add is counted once under any interleaving.
// A workgroup adds at most 2^31 records to its table before it flushes, so that n fits its 32 bits and S its 64.
#include <hip/hip_runtime.h>

#include <math.h>

#include "align_dev.h"
#include "dtw_dev.h"
#include "model_dev.h"
#include "wave_prims.h"

namespace unc {
namespace {

struct ModelBins {
    unsigned long long S[UNC_NKMER], lo[UNC_NKMER], hi[UNC_NKMER];
    uint32_t n[UNC_NKMER];
    uint32_t dropped;
};

__device__ inline void bins_clear(ModelBins &B) {
    for (uint32_t k = threadIdx.x; k < (uint32_t)UNC_NKMER; k += MODEL_BLOCK) { B.S[k] = 0; B.lo[k] = 0; B.hi[k] = 0; B.n[k] = 0; }
    if (threadIdx.x == 0) B.dropped = 0;
    __syncthreads();
}

// one record into the workgroup's table
__device__ inline void bins_add(ModelBins &B, uint32_t flags, uint32_t kmer, float level, uint32_t shared) {
    if (shared && !(flags & UNC_MODEL_KEEP_SHARED)) return;
    // not finite, or |level| >= 2048 (a NaN compares false: the exponent test comes first)
    if ((__float_as_uint(level) & 0x7F800000u) == 0x7F800000u || !(fabsf(level) < MODEL_LEVEL_LIMIT)) {
        atomicAdd(&B.dropped, 1u);
        return;
    }
    UNC_SIM_CHECK(kmer < (uint32_t)UNC_NKMER);
    if (kmer >= (uint32_t)UNC_NKMER) return;            // (cannot happen: the host has checked the k-mers)
    const double scaled = (double)level * MODEL_Q_ONE;  // exact: a float times a power of two
    const long long q = llrint(scaled);                 // round to nearest even
    const unsigned long long qq = (unsigned long long)(q * q);
    atomicAdd(&B.n[kmer], 1u);
    atomicAdd(&B.S[kmer], (unsigned long long)q);       // two's complement: the sum of the words is the word of the sum
    const unsigned long long old = atomicAdd(&B.lo[kmer], qq);
    if (old + qq < old) atomicAdd(&B.hi[kmer], 1ull);
}

// the table's bins that hold something -> the accumulator, and the table is empty again
__device__ inline void bins_flush(ModelBins &B, unsigned long long *acc) {
    __syncthreads();
    for (uint32_t k = threadIdx.x; k < (uint32_t)UNC_NKMER; k += MODEL_BLOCK) {
        const uint32_t n = B.n[k];
        if (n == 0) continue;
        atomicAdd(acc + MODEL_ACC_N + k, (unsigned long long)n);
        atomicAdd(acc + MODEL_ACC_S + k, B.S[k]);
        const unsigned long long x = B.lo[k];
        const unsigned long long old = atomicAdd(acc + MODEL_ACC_LO + k, x);
        const unsigned long long carry = old + x < old ? 1ull : 0ull;
        const unsigned long long h = B.hi[k] + carry;
        if (h) atomicAdd(acc + MODEL_ACC_HI + k, h);
        B.S[k] = 0; B.lo[k] = 0; B.hi[k] = 0; B.n[k] = 0;
    }
    if (threadIdx.x == 0) {
        if (B.dropped) atomicAdd(acc + MODEL_ACC_DROPPED, (unsigned long long)B.dropped);
        B.dropped = 0;
    }
    __syncthreads();
}

// One launch: the caller's arrays (A.jobs == null: workgroup b takes records [b, b + 1) * MODEL_RECS_PER_BLOCK), or a round's records
// where k_align_segments left them (workgroup b takes every gridDim.x-th alignment of the round; record s of query q belongs to
// k-mer kmers[km_off + row_first + s]).  The choice is uniform over the grid
__global__ void __launch_bounds__(MODEL_BLOCK) k_model_accum(ModelAccum A) {
    __shared__ ModelBins B;
    bins_clear(B);
    if (!A.jobs) {
        const uint64_t lo = (uint64_t)blockIdx.x * MODEL_RECS_PER_BLOCK;
        const uint64_t hi = lo + MODEL_RECS_PER_BLOCK < A.n ? lo + MODEL_RECS_PER_BLOCK : A.n;
        for (uint64_t i = lo + threadIdx.x; i < hi; i += MODEL_BLOCK) bins_add(B, A.flags, A.kmers[i], A.levels[i], A.shared ? A.shared[i] : 0u);
        bins_flush(B, A.acc);
        return;
    }
    uint32_t added = 0;             // (uniform over the workgroup) records since the last flush
    for (uint32_t a = blockIdx.x; a < A.n_jobs; a += gridDim.x) {
        const uint32_t q = A.jobs[a].out;
        const unc_seg_info_t inf = A.info[q];
        if (inf.status == UNC_SEG_NONE) continue;
        const AlignQuery Q = A.queries[q];
        const uint64_t room = A.seg_off[q + 1] - A.seg_off[q];
        UNC_SIM_CHECK((uint64_t)inf.n_rows <= room && (uint64_t)inf.row_first + inf.n_rows <= Q.n_km);
        uint32_t n = (uint64_t)inf.n_rows < room ? inf.n_rows : (uint32_t)room;
        if ((uint64_t)inf.row_first + n > Q.n_km) n = inf.row_first < Q.n_km ? Q.n_km - inf.row_first : 0;       // (cannot happen)
        if ((uint64_t)added + n > MODEL_FLUSH_RECS) { bins_flush(B, A.acc); added = 0; }
        added += n;
        const unc_segment_t *seg = A.seg + A.seg_off[q];
        const uint16_t *km = A.kmers + Q.km_off + inf.row_first;
        for (uint32_t s = threadIdx.x; s < n; s += MODEL_BLOCK) bins_add(B, A.flags, km[s], seg[s].level, seg[s].shared);
    }
    bins_flush(B, A.acc);
}

}  // namespace

// the grid goes by the record count: a workgroup for every MODEL_RECS_PER_BLOCK records (of a round: at most one per alignment)
void launch_model_accum(const ModelAccum &a, uint64_t n_records, hipStream_t st) {
    uint64_t grid = (n_records + MODEL_RECS_PER_BLOCK - 1) / MODEL_RECS_PER_BLOCK;
    if (a.jobs && grid > a.n_jobs) grid = a.n_jobs;
    if (grid == 0) return;
    hipLaunchKernelGGL(k_model_accum, dim3((uint32_t)grid), dim3(MODEL_BLOCK), 0, st, a);
}

}  // namespace unc
