// What unc_dtw.cpp (host) and k_dtw.hip (kernel) share: the job record of one alignment and the launch wrapper.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/uncalled_hip.h"

struct unc_model;

namespace unc {

constexpr uint32_t DTW_LANES = 64;          // rows of a strip: one per lane
constexpr uint32_t DTW_CRUMBS_PER_WORD = 16;
constexpr int DTW_MAX_DEVICES = 64;         // devices the per-device copy of the model is kept for

// Back-pointers of one alignment: strips of 64 rows, each swept in cols + 63 steps (lane l is at column t - l in step t).  A strip's
// steps are cut into blocks of 16; a block is 64 words, lane l's word holds its 16 moves of the block at 2 bits each: one
// coalesced 256-byte store per 16 steps.
__host__ __device__ inline uint64_t dtw_step_blocks(uint32_t cols) { return ((uint64_t)cols + 63 + 15) / 16; }
__host__ __device__ inline uint64_t dtw_strips(uint32_t rows) { return ((uint64_t)rows + 63) / 64; }
__host__ __device__ inline uint64_t dtw_crumb_words(uint32_t rows, uint32_t cols) { return dtw_strips(rows) * dtw_step_blocks(cols) * 64; }
// a line = one row of scores (the last row of a strip, handed to the next strip), padded to whole blocks of 64 columns
__host__ __device__ inline uint64_t dtw_line_floats(uint32_t cols) { return ((uint64_t)cols + 63) / 64 * 64; }

// ---- the band (include/uncalled_hip.h): cell (i, j) is in the band iff i + W >= c(j) and i <= c(j) + W, c(j) = floor(j * rows / cols).
// Host (planner) and kernel share every formula of the banded layout, so that what one allocates is what the other addresses.
// the half-width the layout works with: at W >= rows every cell is in the band already
__host__ __device__ inline uint32_t dtw_band_eff(uint32_t rows, uint32_t band) { return band < rows ? band : rows; }
// the band holds (rows - 1, cols - 1) and a connected monotone path iff ceil(rows / cols) <= W + 1
__host__ __device__ inline bool dtw_band_feasible(uint32_t rows, uint32_t cols, uint32_t band) {
    return ((uint64_t)rows + cols - 1) / cols <= (uint64_t)band + 1;
}
// row i's columns in the band are [lo, hi] (c is non-decreasing); lo > hi: none.  W = dtw_band_eff(): the products stay below 2^64
__host__ __device__ inline uint32_t dtw_band_lo(uint32_t i, uint32_t rows, uint32_t cols, uint32_t W) {
    if (i <= W) return 0;                                                       // c(0) = 0 >= i - W
    return (uint32_t)(((uint64_t)(i - W) * cols + rows - 1) / rows);            // the first j with j * rows >= (i - W) * cols
}
__host__ __device__ inline uint32_t dtw_band_hi(uint32_t i, uint32_t rows, uint32_t cols, uint32_t W) {
    const uint64_t past = (((uint64_t)i + W + 1) * cols + rows - 1) / rows;     // the first j with j * rows >= (i + W + 1) * cols
    return (uint32_t)(past < cols ? past : cols) - 1;
}
// A strip of 64 rows sweeps the union of its rows' intervals, [lo(first row), hi(last row)]: at most this many columns, since
// hi(i + 63) - lo(i) + 1 < (64 + 2 W) * cols / rows + 2.  Every strip gets the same room: (width + 63 steps of skew) in blocks of 16
__host__ __device__ inline uint64_t dtw_band_width(uint32_t rows, uint32_t cols, uint32_t W) {
    const uint64_t w = (64 + 2 * (uint64_t)W) * cols / rows + 2;
    return w < cols ? w : cols;
}
__host__ __device__ inline uint64_t dtw_band_step_blocks(uint32_t rows, uint32_t cols, uint32_t W) {
    return (dtw_band_width(rows, cols, W) + 63 + 15) / 16;
}
__host__ __device__ inline uint64_t dtw_band_crumb_words(uint32_t rows, uint32_t cols, uint32_t W) {
    return dtw_strips(rows) * dtw_band_step_blocks(rows, cols, W) * 64;
}
// steps of one wavefront's dependent chain: what the queue is ordered by
__host__ __device__ inline uint64_t dtw_band_steps(uint32_t rows, uint32_t cols, uint32_t W) {
    return dtw_strips(rows) * (dtw_band_width(rows, cols, W) + 63);
}

// ---- the adaptive band (unc_dtw_adapt_batch, include/uncalled_hip.h): B rows per anti-diagonal, B / 64 cells per lane.  Per block
// of 16 anti-diagonals one word per band cell (cell c of lane l: word (block * B / 64 + c) * 64 + l), then lo_d as int32 per
// anti-diagonal, padded to whole blocks of 64: about (rows + cols) * (B / 4 + 4) bytes.
__host__ __device__ inline bool dtw_adapt_band_ok(uint32_t B) { return B == 64 || B == 128 || B == 256; }
__host__ __device__ inline uint64_t dtw_adapt_diags(uint32_t rows, uint32_t cols) { return (uint64_t)rows + cols - 1; }
// the first word of lo_d = the words of back-pointers
__host__ __device__ inline uint64_t dtw_adapt_lo_first(uint32_t rows, uint32_t cols, uint32_t B) {
    return (dtw_adapt_diags(rows, cols) + 15) / 16 * B;
}
__host__ __device__ inline uint64_t dtw_adapt_words(uint32_t rows, uint32_t cols, uint32_t B) {
    return dtw_adapt_lo_first(rows, cols, B) + (dtw_adapt_diags(rows, cols) + 63) / 64 * 64;
}

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
    const DtwJob *jobs;           // descending cell count (with a band: descending steps)
    uint32_t n_jobs;
    uint32_t subseq;
    uint32_t band;                // 0: the full matrix; else the half-width W, subseq is UNC_DTW_NONE, and crumb_off is of the banded layout
    uint32_t adaptive;            // != 0: band is the adaptive width B (dtw_adapt_band_ok), crumb_off is of the adaptive layout, no lines
    float dw, hw, vw;
    uint32_t *crumbs;
    float *lines;
    uint32_t *path;               // nullptr: no paths wanted
    unc_dtw_result_t *res;
    uint32_t *next;               // the queue: index of the next job to take
};

void launch_dtw(const DtwBatch &b, uint32_t cost, uint32_t grid, hipStream_t st);

// unc_dtw.cpp: what unc_dtw_batch does once its columns and k-mers are in device memory -- the queue in descending cell count, the
// rounds that fit the workspace, the launches and the copies of results and paths to the host.  jobs[a] names alignment a's first
// column and first k-mer in d_events / d_kmers, its rows and columns, path_cap and out = a (the three offsets of a round are filled
// here).  skip (may be null): alignments with skip[a] != 0 are left out and res[a] is not written.  The arguments are the caller's
// to check.  band: 0 = the full matrix, else the half-width: back-pointers, rounds, UNC_DTW_TOO_LARGE and the queue (descending steps)
// go by the banded layout, and an alignment whose band is too narrow gets UNC_DTW_BAND_TOO_NARROW.  unc_align.cpp hands over the levels its own kernels have written: they never visit the host.
// hook (may be null): every alignment's path is then kept whole on the device (rows + cols - 1 pairs of room, whatever the caller's),
// and after each round's kernel, before anything is copied out and the next round reuses the buffers, the hook is handed the round.
// What the caller gets is as without it: path_cap pairs at most, and UNC_DTW_PATH_TRUNCATED by path_cap.
// model (may be null: the template's, kept per device for the life of the process): whose tables the costs are read from.
// adaptive: band is the adaptive width B (the caller has checked dtw_adapt_band_ok and a global alignment): the adaptive layout,
// the queue in descending anti-diagonals, no UNC_DTW_BAND_TOO_NARROW.
struct DtwRoundHook {
    virtual ~DtwRoundHook() = default;
    // d_jobs: the round's jobs as the kernel saw them (path_cap = rows + cols - 1); n_rows: the sum of their rows; d_res is indexed
    // by DtwJob::out
    virtual int round(const DtwJob *d_jobs, uint32_t n_jobs, uint64_t n_rows, const uint32_t *d_path, const unc_dtw_result_t *d_res, hipStream_t st) = 0;
};
int dtw_run_device(int device, uint32_t n, const float *d_events, const uint16_t *d_kmers, const DtwJob *jobs, const uint8_t *skip,
                   const unc_dtw_params_t *prm, uint32_t band, uint64_t workspace_bytes, unc_dtw_result_t *res, uint32_t *path,
                   const uint64_t *path_off, hipStream_t st, DtwRoundHook *hook = nullptr, const unc_model *model = nullptr,
                   bool adaptive = false);
// the template model's 3 x 1024 floats on `device` (uploaded once per device) and on the host; dtw_model_default: with its mean and
// deviation over all k-mers (unc_model.h)
int dtw_model_device(int device, const float **out);
const float *dtw_model_host();
struct ModelTables;
const ModelTables &dtw_model_default();
}  // namespace unc
