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

// ---- the layout in force, said once: which of the three kernels runs and its width.  What the host plans by goes through these
// members; the kernels call the formulas above directly.
enum class DtwKind : uint32_t { Full, Band, Adapt };      // k_dtw, k_dtw_band, k_dtw_adapt
struct DtwLayout {
    uint32_t width;               // Band: the half-width W; Adapt: the width B; Full: 0.  (First: where k_dtw_band has always read it)
    DtwKind kind;
    static DtwLayout full() { return {0, DtwKind::Full}; }
    static DtwLayout band(uint32_t W) { return {W, DtwKind::Band}; }
    static DtwLayout adapt(uint32_t B) { return {B, DtwKind::Adapt}; }
    // steps of one wavefront's dependent chain: what the queue is ordered by
    uint64_t chain(uint32_t rows, uint32_t cols) const {
        return kind == DtwKind::Band ? dtw_band_steps(rows, cols, dtw_band_eff(rows, width))
             : kind == DtwKind::Adapt ? dtw_adapt_diags(rows, cols) : (uint64_t)rows * cols;
    }
    // 32-bit words of one alignment's back-pointers (Adapt: and of its lo_d)
    uint64_t words(uint32_t rows, uint32_t cols) const {
        return kind == DtwKind::Band ? dtw_band_crumb_words(rows, cols, dtw_band_eff(rows, width))
             : kind == DtwKind::Adapt ? dtw_adapt_words(rows, cols, width) : dtw_crumb_words(rows, cols);
    }
    // floats of one alignment's two lines
    uint64_t line_floats(uint32_t cols) const { return kind == DtwKind::Adapt ? 0 : 2 * dtw_line_floats(cols); }
    // false: the alignment gets UNC_DTW_BAND_TOO_NARROW and is not computed
    bool feasible(uint32_t rows, uint32_t cols) const { return kind != DtwKind::Band || dtw_band_feasible(rows, cols, width); }
};
// The rules of a layout that a caller's arguments break (0: none), for the entry points to report in their own order and words.
// DTW_MODE_WIDTH: a Band of 0, an Adapt not of 64, 128 or 256.  DTW_MODE_SUBSEQ: a band of either sort is global only, so a Band
// or an Adapt with UNC_DTW_ROW or UNC_DTW_COL (an unknown subseq is the caller's to report, and a width of 0 is DTW_MODE_WIDTH's).
enum : uint32_t { DTW_MODE_WIDTH = 1, DTW_MODE_SUBSEQ = 2 };
inline uint32_t dtw_mode_faults(DtwLayout L, uint32_t subseq) {
    const bool width_ok = L.kind == DtwKind::Full || (L.kind == DtwKind::Band ? L.width != 0 : dtw_adapt_band_ok(L.width));
    const bool subseq_ok = L.kind == DtwKind::Full || L.width == 0 || subseq == UNC_DTW_NONE || subseq > UNC_DTW_COL;
    return (width_ok ? 0u : DTW_MODE_WIDTH) | (subseq_ok ? 0u : DTW_MODE_SUBSEQ);
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
    const DtwJob *jobs;           // descending DtwLayout::chain
    uint32_t n_jobs;
    uint32_t subseq;              // (with a band of either sort: UNC_DTW_NONE)
    DtwLayout layout;             // what crumb_off and line_off are of; launch_dtw picks the kernel by it
    float dw, hw, vw;
    uint32_t *crumbs;
    float *lines;
    uint32_t *path;               // nullptr: no paths wanted
    unc_dtw_result_t *res;
    uint32_t *next;               // the queue: index of the next job to take
};

void launch_dtw(const DtwBatch &b, uint32_t cost, uint32_t grid, hipStream_t st);

// hook: every alignment's path is kept whole on the device (rows + cols - 1 pairs of room, whatever the caller's), and after each
// round's kernel, before anything is copied out and the next round reuses the buffers, the hook is handed the round.  What the caller
// gets is as without it: path_cap pairs at most, and UNC_DTW_PATH_TRUNCATED by path_cap.
struct DtwRoundHook {
    virtual ~DtwRoundHook() = default;
    // d_jobs: the round's jobs as the kernel saw them (path_cap = rows + cols - 1); n_rows: the sum of their rows; d_res is indexed
    // by DtwJob::out
    virtual int round(const DtwJob *d_jobs, uint32_t n_jobs, uint64_t n_rows, const uint32_t *d_path, const unc_dtw_result_t *d_res, hipStream_t st) = 0;
};

// unc_dtw.cpp: what unc_dtw_batch does once its columns and k-mers are in device memory -- the queue in descending chain, the rounds
// that fit the workspace, the launches and the copies of results and paths to the host.  The fields are the caller's to check
// (dtw_mode_faults among the checks).  unc_align.cpp hands over the levels its own kernels have written: they never visit the host.
struct DtwCall {
    int device;                     // where everything below lies
    hipStream_t st;                 // every copy and launch is queued here
    uint32_t n;                     // alignments
    const float *d_events;          // the batch's columns, on the device
    const uint16_t *d_kmers;        // the batch's k-mers, on the device
    const DtwJob *jobs;             // [n], host: first column and k-mer, rows, cols, path_cap, out = a (a round's three offsets are filled here)
    const uint8_t *skip;            // null, or [n]: skip[a] != 0 leaves alignment a out and res[a] unwritten
    const unc_dtw_params_t *prm;    // subseq, cost and the three weights
    DtwLayout layout;               // which kernel, and what the queue, the rounds and UNC_DTW_TOO_LARGE go by
    uint64_t workspace_bytes;       // back-pointers a round may hold; 0: half of the free device memory
    unc_dtw_result_t *res;          // [n], host
    uint32_t *path;                 // null (no paths wanted), or the caller's pairs on the host
    const uint64_t *path_off;       // (with path) [n + 1]: alignment a's room is [path_off[a], path_off[a + 1])
    DtwRoundHook *hook;             // null, or handed every round (above)
    const unc_model *model;         // whose tables the costs are read from; null: the template's, kept per device for the life of the process
};
int dtw_run_device(const DtwCall &c);
// the template model's 3 x 1024 floats on `device` (uploaded once per device) and on the host; dtw_model_default: with its mean and
// deviation over all k-mers (unc_model.h)
int dtw_model_device(int device, const float **out);
const float *dtw_model_host();
struct ModelTables;
const ModelTables &dtw_model_default();
}  // namespace unc
