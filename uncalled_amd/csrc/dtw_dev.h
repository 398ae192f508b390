// What unc_dtw.cpp (host) and k_dtw.hip (kernel) share: the job record of one alignment and the launch wrapper.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/uncalled_hip.h"

namespace unc {

constexpr uint32_t DTW_LANES = 64;          // rows of a strip: one per lane
constexpr uint32_t DTW_CRUMBS_PER_WORD = 16;

// Back-pointers of one alignment: strips of 64 rows, each swept in cols + 63 steps (lane l is at column t - l in step t).  A strip's
// steps are cut into blocks of 16; a block is 64 words, lane l's word holds its 16 moves of the block at 2 bits each: one
// coalesced 256-byte store per 16 steps.
__host__ __device__ inline uint64_t dtw_step_blocks(uint32_t cols) { return ((uint64_t)cols + 63 + 15) / 16; }
__host__ __device__ inline uint64_t dtw_strips(uint32_t rows) { return ((uint64_t)rows + 63) / 64; }
__host__ __device__ inline uint64_t dtw_crumb_words(uint32_t rows, uint32_t cols) { return dtw_strips(rows) * dtw_step_blocks(cols) * 64; }
// a line = one row of scores (the last row of a strip, handed to the next strip), padded to whole blocks of 64 columns
__host__ __device__ inline uint64_t dtw_line_floats(uint32_t cols) { return ((uint64_t)cols + 63) / 64 * 64; }

struct DtwJob {
    uint64_t ev_off, km_off;      // first event / k-mer in the batch's arrays
    uint64_t crumb_off;           // first word of the alignment's back-pointers
    uint64_t line_off;            // first float of its two lines
    uint64_t path_off;            // first pair of its path in the round's path buffer
    uint32_t rows, cols;          // k-mers, events
    uint32_t path_cap;            // pairs it may write
    uint32_t out;                 // index of its result
};

struct DtwBatch {
    const float *events;
    const uint16_t *kmers;
    const float *model;           // [3][1024]: mean, 2 * stdv^2, log(sqrt(pi * that)) of the template model
    const DtwJob *jobs;           // descending cell count
    uint32_t n_jobs;
    uint32_t subseq;
    float dw, hw, vw;
    uint32_t *crumbs;
    float *lines;
    uint32_t *path;               // nullptr: no paths wanted
    unc_dtw_result_t *res;
    uint32_t *next;               // the queue: index of the next job to take
};

void launch_dtw(const DtwBatch &b, uint32_t cost, uint32_t grid, hipStream_t st);
}  // namespace unc
