// What unc_model_acc.cpp and unc_align.cpp (host) and k_model.hip (kernel) share: the accumulator's layout in global memory, the kernel's constants and
// its argument record.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/uncalled_hip.h"
#include "align_dev.h"

namespace unc {

constexpr uint32_t MODEL_BLOCK = 256;                   // lanes of a workgroup
constexpr uint32_t MODEL_RECS_PER_BLOCK = 4096;         // the grid rule: one workgroup for this many records (16 a lane)
constexpr uint32_t MODEL_FLUSH_RECS = 1u << 31;         // records a workgroup's table takes between two flushes
constexpr float MODEL_LEVEL_LIMIT = 2048.0f;            // |level| at and above it is dropped: q * q stays below 2^62
constexpr double MODEL_Q_ONE = 1048576.0;               // 2^20: q = llrint(level * MODEL_Q_ONE)

// the accumulator: 4 x 1024 words and one, in this order
constexpr uint32_t MODEL_ACC_N = 0, MODEL_ACC_S = UNC_NKMER, MODEL_ACC_LO = 2 * UNC_NKMER, MODEL_ACC_HI = 3 * UNC_NKMER;
constexpr uint32_t MODEL_ACC_DROPPED = 4 * UNC_NKMER, MODEL_ACC_WORDS = 4 * UNC_NKMER + 1;

struct DtwJob;
struct ModelAccum {
    unsigned long long *acc;      // MODEL_ACC_WORDS
    uint32_t flags;               // UNC_MODEL_*
    uint32_t n_jobs;
    // the caller's arrays (jobs == null): record i is (kmers[i], levels[i], shared[i]); shared may be null (all 0)
    uint64_t n;
    const float *levels;
    const uint32_t *shared;
    const uint16_t *kmers;        // with jobs: the batch's rows, query q's from queries[q].km_off on
    // a round of the alignment (k_align_segments has run on it): everything by DtwJob::out, as in SegArgs
    const DtwJob *jobs;
    const unc_seg_info_t *info;
    const AlignQuery *queries;
    const uint64_t *seg_off;
    const unc_segment_t *seg;
};
// n_records: the arrays' n, or the sum of the round's alignments' rows (a bound on its records)
void launch_model_accum(const ModelAccum &a, uint64_t n_records, hipStream_t st);
}  // namespace unc
