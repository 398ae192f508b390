// Batched full-matrix dynamic time warping of event means against reference k-mers: DTW<float, u16, Func>::compute_matrix and
// ::traceback (src/dtw.hpp:51-120) with the costs of DTWr94p / DTWr94d (dtw.hpp:188-214).  (dtw_band_one, further down, is the same
// arithmetic on the cells of a band around the diagonal.)
//
// One wavefront per alignment, alignments taken from a queue in descending cell count.  The matrix is swept in strips of 64 rows
// (k-mers), one row per lane, skewed: in step t lane l computes column t - l, so that its three predecessors are its own last
// value (H), the value lane l - 1 computed one step ago (V) and the one it computed two steps ago (D).  Events enter at lane 0 and
// move one lane per step; lane 0 takes V and D from the last row of the strip above.  A cell is min over three of
// float + float * float with the reference's tie rule, so the sweep order cannot change a bit of the result.
//
// Scores stay in registers.  What reaches memory: the back-pointers at 2 bits per cell (lane l's 16 moves of a block of 16 steps
// are one word: a coalesced 256-byte store per 16 steps), and ONE row of scores per strip -- the line the next strip's lane 0 reads,
// 4 bytes per 64 cells, two lines per alignment used in turn.  After the last strip that line is the matrix's last row, which
// DTWSubSeq::COL scans for the end cell; DTWSubSeq::ROW needs the last column, which every lane sees in its own register.
// The traceback runs on the same wavefront over the packed back-pointers and writes the path 64 pairs at a time.
#include <hip/hip_runtime.h>

#include <float.h>
#include <math.h>

#include "dtw_dev.h"
#include "wave_prims.h"

namespace unc {
namespace {

constexpr float DTW_MAX_COST = FLT_MAX / 2.0f;      // dtw.hpp:148
constexpr uint32_t DTW_NONE_IDX = 0xFFFFFFFFu;
enum : uint32_t { MOVE_D = 0, MOVE_H = 1, MOVE_V = 2 };   // dtw.hpp:147

// the value lane `src` holds (src: wave-uniform)
__device__ __forceinline__ uint32_t lane_value(uint32_t v, uint32_t src) { return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)src); }
__device__ __forceinline__ float lane_value(float v, uint32_t src) { return __uint_as_float(lane_value(__float_as_uint(v), src)); }

template <int COST> __device__ __forceinline__ float dtw_cost(float e, float mu, float v2, float ln) {
    const float d = __fsub_rn(e, mu);
    if (COST == (int)UNC_DTW_R94D) return fabsf(d);                            // dtw.hpp:212-214
    const double q = -((double)d * (double)d) / (double)v2 - (double)ln;        // pore_model.hpp:163-165
    return -(float)q;                                                           // dtw.hpp:188-190
}

// (value, index) of the first smallest element over the wave; index DTW_NONE_IDX = the lane has none
__device__ __forceinline__ void wave_first_min(float &v, uint32_t &idx) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const float ov = __shfl_xor(v, d);
        const uint32_t oi = (uint32_t)__shfl_xor((int)idx, d);
        if (oi != DTW_NONE_IDX && (idx == DTW_NONE_IDX || ov < v || (ov == v && oi < idx))) { v = ov; idx = oi; }
    }
}

// ---- the leaves that the three sweeps share (dtw_one and dtw_band_one here, dtw_adapt_one of k_dtw_adapt.hip): no loop of their own,
// scalars in and scalars out -- an element of a per-lane array is handed over by value (pick4, k_dtw_adapt.hip).

// one k-mer's row of the model's three tables
struct ModelRow { float mu, v2, ln; };
__device__ __forceinline__ ModelRow model_row(const float *model, uint32_t k) { return {model[k], model[1024 + k], model[2048 + k]}; }

// a cell from its three predecessors, dtw.hpp:57-71: the three sums, and the reference's tie order D <= H, D <= V; H <= V
struct DtwCell { float m; uint32_t mv; };
__device__ __forceinline__ DtwCell dtw_cell(float dp, float hp, float vp, float cost, float dw, float hw, float vw) {
    const float ds = __fadd_rn(dp, __fmul_rn(dw, cost));
    const float hs = __fadd_rn(hp, __fmul_rn(hw, cost));
    const float vs = __fadd_rn(vp, __fmul_rn(vw, cost));
    if (ds <= hs && ds <= vs) return {ds, MOVE_D};
    if (hs <= vs) return {hs, MOVE_H};
    return {vs, MOVE_V};
}

// (Two pieces stay in the three tracebacks, because as helpers they changed the code around them and cost some kernel time: the step
// from a move to the next (i, j), and the staging of the path 64 pairs at a time -- DESIGN.md, "Shared leaves")

// the result, by lane 0.  mean_score: the host divides (score / (float)path_len, dtw.hpp:130-132)
__device__ __forceinline__ void dtw_write_result(const DtwBatch &B, const DtwJob &J, float score, uint64_t path_len, uint32_t status) {
    if (lane_id() == 0) B.res[J.out] = unc_dtw_result_t{score, 0.0f, path_len, status, 0};
}

// the queue: the index of the wavefront's next job; B.n_jobs or more: none is left.  (The index, not the job: a job filled in through
// a reference cost the full-matrix kernel 10 VGPRs and two waves per SIMD)
__device__ __forceinline__ uint32_t dtw_take_job(const DtwBatch &B) {
    uint32_t q = 0;
    if (lane_id() == 0) q = atomicAdd(B.next, 1u);
    return uniform32(q);
}

template <int COST> __device__ void dtw_one(const DtwBatch &B, const DtwJob &J) {
    const uint32_t lane = (uint32_t)lane_id();
    const uint32_t rows = uniform32(J.rows), cols = uniform32(J.cols);
    const bool row_mode = B.subseq == UNC_DTW_ROW, col_mode = B.subseq == UNC_DTW_COL;
    const float hinit = row_mode ? 0.0f : DTW_MAX_COST;       // hscore(i, 0), dtw.hpp:161-165
    const float vinit = col_mode ? 0.0f : DTW_MAX_COST;       // vscore(0, j) and dscore(0, j > 0), :167-179
    const float dinit = row_mode ? 0.0f : DTW_MAX_COST;       // dscore(i > 0, 0)
    const float dw = B.dw, hw = B.hw, vw = B.vw;
    const float *ev = B.events + J.ev_off;
    const uint16_t *km = B.kmers + J.km_off;
    uint32_t *crumbs = B.crumbs + J.crumb_off;
    const uint64_t line_floats = dtw_line_floats(cols);
    float *line0 = B.lines + J.line_off, *line1 = line0 + line_floats;
    const uint32_t n_strips = (uint32_t)dtw_strips(rows), n_blocks = (uint32_t)dtw_step_blocks(cols);
    const uint32_t n_steps = cols + 63;

    // ROW: the first smallest score of the last column among this lane's rows.  A candidate is a score that compared smaller, as in
    // the reference's scan, here and in the COL scan below.  Only there can it matter: a NaN event makes its whole column NaN and
    // no other, so the last column holds NaN in every row or in none, while the last row may hold one in a lane's first cell,
    // where no later comparison could replace it
    float best_v = INFINITY;
    uint32_t best_i = DTW_NONE_IDX;
    float last_score = 0.0f;                // the matrix's last cell
    const float *last_row = line0;

    for (uint32_t s = 0; s < n_strips; ++s) {
        const uint32_t i = s * 64 + lane;
        const bool row_ok = i < rows;
        const uint32_t last_lane = rows - 1 - s * 64 < 63u ? rows - 1 - s * 64 : 63u;     // the strip's last row
        const float *lin = (s & 1u) ? line0 : line1;        // what strip s - 1 wrote
        float *lout = (s & 1u) ? line1 : line0;
        float mu = 0.0f, v2 = 1.0f, ln = 0.0f;
        if (row_ok) {
            const ModelRow r = model_row(B.model, km[i]);
            mu = r.mu; v2 = r.v2; ln = r.ln;
        }
        float cur = hinit;                                  // the lane's last value: H of its next cell
        float prev_up = i == 0 ? 0.0f : dinit;              // the V it took one step ago: D of its next cell
        float e = 0.0f, ev_reg = 0.0f, in_reg = vinit, out_reg = 0.0f;
        uint32_t cw = 0;
        uint32_t *cstrip = crumbs + (uint64_t)s * n_blocks * 64;
        for (uint32_t t = 0; t < n_steps; ++t) {
            const uint32_t u = t & 63u;
            if (u == 0) {       // the next 64 events, and the 64 scores above them
                const uint32_t c = t + lane;
                ev_reg = c < cols ? ev[c] : 0.0f;
                if (s > 0) in_reg = c < cols ? lin[c] : 0.0f;
            }
            float e_in = __shfl_up(e, 1), up = __shfl_up(cur, 1);
            const float e0 = lane_value(ev_reg, u), up0 = lane_value(in_reg, u);
            if (lane == 0) { e_in = e0; up = up0; }
            e = e_in;
            const bool act = row_ok && t >= lane && t - lane < cols;
            const DtwCell c = dtw_cell(prev_up, cur, up, dtw_cost<COST>(e, mu, v2, ln), dw, hw, vw);
            if (act) { prev_up = up; cur = c.m; cw |= c.mv << (2u * (t & 15u)); }
            if ((t & 15u) == 15u || t == n_steps - 1) {
                UNC_SIM_CHECK((uint64_t)s * n_blocks * 64 + (uint64_t)(t >> 4) * 64 + lane < dtw_crumb_words(rows, cols));
                cstrip[(uint64_t)(t >> 4) * 64 + lane] = cw;
                cw = 0;
            }
            // the strip's last row, gathered 64 columns at a time for the strip below
            const float lv = lane_value(cur, last_lane);
            if (t >= last_lane && t - last_lane < cols) {
                const uint32_t jl = t - last_lane;
                if (lane == (jl & 63u)) out_reg = lv;
                if (((jl & 63u) == 63u || jl == cols - 1) && lane <= (jl & 63u)) {
                    UNC_SIM_CHECK((jl & ~63u) + lane < cols);
                    lout[(jl & ~63u) + lane] = out_reg;
                }
            }
        }
        if (row_mode && row_ok && cur < best_v) { best_v = cur; best_i = i; }     // cur = M(i, cols - 1)
        if (s == n_strips - 1) { last_score = lane_value(cur, last_lane); last_row = lout; }
        // lanes read what other lanes wrote: the line in the next strip, the back-pointers in the traceback
        __threadfence();
    }

    // the end cell, dtw.hpp:77-98: the first strictly smaller score wins, scanning upward from a start at the last cell
    uint32_t ei = rows - 1, ej = cols - 1;
    float score = last_score;
    if (row_mode) {
        wave_first_min(best_v, best_i);
        if (best_i != DTW_NONE_IDX && best_v < last_score) { score = best_v; ei = best_i; }
    } else if (col_mode) {
        float bv = INFINITY;
        uint32_t bj = DTW_NONE_IDX;
        for (uint32_t j = lane; j < cols; j += 64) {
            const float v = last_row[j];
            if (v < bv) { bv = v; bj = j; }
        }
        wave_first_min(bv, bj);
        if (bj != DTW_NONE_IDX && bv < last_score) { score = bv; ej = bj; }
    }
    ei = uniform32(ei); ej = uniform32(ej);
    score = __uint_as_float(uniform32(__float_as_uint(score)));

    // traceback, dtw.hpp:100-119.  (i, j) is wave-uniform; the block of back-pointers it lies in is held one word per lane
    const bool want_path = B.path != nullptr;
    const uint32_t cap = J.path_cap;
    uint2 *path = want_path ? reinterpret_cast<uint2 *>(B.path) + J.path_off : nullptr;
    uint32_t i = ei, j = ej, held_s = DTW_NONE_IDX, held_b = DTW_NONE_IDX, w = 0;
    uint32_t pj = 0, pi = 0;
    uint64_t p = 0;
    for (;;) {
        if (lane == (uint32_t)(p & 63u)) { pj = j; pi = i; }
        const bool done = (i == 0 || row_mode) && (j == 0 || col_mode);
        if ((p & 63u) == 63u || done) {
            const uint64_t at = (p & ~(uint64_t)63) + lane;
            if (want_path && lane <= (uint32_t)(p & 63u) && at < cap) path[at] = make_uint2(pj, pi);
        }
        ++p;
        if (done) break;
        const uint32_t s = i >> 6, l = i & 63u, t = j + l, b = t >> 4;
        if (s != held_s || b != held_b) {
            w = crumbs[((uint64_t)s * n_blocks + b) * 64 + lane];
            held_s = s; held_b = b;
        }
        const uint32_t mv = (lane_value(w, l) >> (2u * (t & 15u))) & 3u;
        if (i == 0 || (mv == MOVE_H && j > 0)) --j;
        else if (j == 0 || mv == MOVE_V) --i;
        else { --i; --j; }
    }
    dtw_write_result(B, J, score, p, want_path && p > cap ? UNC_DTW_PATH_TRUNCATED : UNC_DTW_OK);
}

template <int COST> __global__ void __launch_bounds__(64) k_dtw(DtwBatch B) {
    for (;;) {
        const uint32_t q = dtw_take_job(B);
        if (q >= B.n_jobs) return;
        const DtwJob J = B.jobs[q];
        dtw_one<COST>(B, J);
        wave_sync();
    }
}

// ---- the band.  The same sweep over fewer cells: cell (i, j) exists iff i + W >= c(j) and i <= c(j) + W, c(j) = floor(j * rows /
// cols); global alignment only.  A row's cells are one column interval [lo, hi], a strip sweeps the union of its rows' intervals,
// [wlo, whi] = [lo(first row), hi(last row)], in whi - wlo + 1 steps plus the skew: in step t lane l is at column wlo + t - l and
// computes iff that lies in its own interval.  A lane outside its interval holds DTW_MAX_COST, the value an absent cell reads as,
// so that H (its own last value), V (lane l - 1's value one step ago) and D (the V of the step before) need no further masking;
// lane 0 masks what it reads from the line by the interval of the row above, because the line holds values of two strips ago at
// the columns the strip above never wrote.  Back-pointers: per strip dtw_band_step_blocks() blocks of 16 steps over its window
// only, step = column - wlo + lane.  The traceback keeps the intervals of the 64 rows of the strip it is in, one per lane, and
// stops before it would read a cell outside them (only non-finite scores lead there).
template <int COST> __device__ void dtw_band_one(const DtwBatch &B, const DtwJob &J) {
    const uint32_t lane = (uint32_t)lane_id();
    const uint32_t rows = uniform32(J.rows), cols = uniform32(J.cols);
    const uint32_t W = dtw_band_eff(rows, uniform32(B.layout.width));
    const float dw = B.dw, hw = B.hw, vw = B.vw;
    const float *ev = B.events + J.ev_off;
    const uint16_t *km = B.kmers + J.km_off;
    uint32_t *crumbs = B.crumbs + J.crumb_off;
    const uint64_t line_floats = dtw_line_floats(cols);
    float *line0 = B.lines + J.line_off, *line1 = line0 + line_floats;
    const uint32_t n_strips = (uint32_t)dtw_strips(rows), n_blocks = (uint32_t)dtw_band_step_blocks(rows, cols, W);

    float score = 0.0f;
    uint32_t plo = 1, phi = 0;              // the interval of the row above the strip (none above the first)
    for (uint32_t s = 0; s < n_strips; ++s) {
        const uint32_t i = s * 64 + lane;
        const bool row_ok = i < rows;
        const uint32_t last_lane = rows - 1 - s * 64 < 63u ? rows - 1 - s * 64 : 63u;
        const float *lin = (s & 1u) ? line0 : line1;
        float *lout = (s & 1u) ? line1 : line0;
        float mu = 0.0f, v2 = 1.0f, ln = 0.0f;
        uint32_t lo = 1, hi = 0;
        if (row_ok) {
            const ModelRow r = model_row(B.model, km[i]);
            mu = r.mu; v2 = r.v2; ln = r.ln;
            lo = dtw_band_lo(i, rows, cols, W); hi = dtw_band_hi(i, rows, cols, W);
        }
        const uint32_t wlo = lane_value(lo, 0), llo = lane_value(lo, last_lane), whi = lane_value(hi, last_lane);
        // (whi >= wlo whenever the band is feasible, and the steps fit the strip's room by dtw_band_width; neither is left to trust)
        uint32_t n_steps = whi >= wlo ? whi - wlo + 1 + last_lane : 0;
        if (n_steps > n_blocks * 16) n_steps = n_blocks * 16;
        float cur = DTW_MAX_COST;
        // D of lane 0's first cell: the matrix's corner, or the cell left of the window in the row above
        float prev_up = DTW_MAX_COST;
        if (lane == 0) {
            if (i == 0) prev_up = 0.0f;
            else if (wlo > 0 && wlo - 1 >= plo && wlo - 1 <= phi) prev_up = lin[wlo - 1];
        }
        float e = 0.0f, ev_reg = 0.0f, in_reg = DTW_MAX_COST, out_reg = 0.0f;
        uint32_t cw = 0;
        uint32_t *cstrip = crumbs + (uint64_t)s * n_blocks * 64;
        for (uint32_t t = 0; t < n_steps; ++t) {
            const uint32_t u = t & 63u;
            if (u == 0) {
                const uint32_t c = wlo + t + lane;
                ev_reg = c < cols ? ev[c] : 0.0f;
                in_reg = c >= plo && c <= phi ? lin[c] : DTW_MAX_COST;
            }
            float e_in = __shfl_up(e, 1), up = __shfl_up(cur, 1);
            const float e0 = lane_value(ev_reg, u), up0 = lane_value(in_reg, u);
            if (lane == 0) { e_in = e0; up = up0; }
            e = e_in;
            const uint32_t j = wlo + t - lane;          // (wraps below the window: then above hi)
            const bool act = t >= lane && j >= lo && j <= hi;
            const DtwCell c = dtw_cell(prev_up, cur, up, dtw_cost<COST>(e, mu, v2, ln), dw, hw, vw);
            prev_up = up;
            cur = act ? c.m : DTW_MAX_COST;
            if (act) cw |= c.mv << (2u * (t & 15u));
            if ((t & 15u) == 15u || t == n_steps - 1) {
                UNC_SIM_CHECK((uint64_t)s * n_blocks * 64 + (uint64_t)(t >> 4) * 64 + lane < dtw_band_crumb_words(rows, cols, W));
                cstrip[(uint64_t)(t >> 4) * 64 + lane] = cw;
                cw = 0;
            }
            // the strip's last row over its own interval, for the strip below
            const float lv = lane_value(cur, last_lane);
            const uint32_t jl = wlo + t - last_lane;
            if (s + 1 < n_strips && t >= last_lane && jl >= llo && jl <= whi) {
                if (lane == (jl & 63u)) out_reg = lv;
                if (((jl & 63u) == 63u || jl == whi) && lane <= (jl & 63u) && (jl & ~63u) + lane >= llo) {
                    UNC_SIM_CHECK((jl & ~63u) + lane < cols);
                    lout[(jl & ~63u) + lane] = out_reg;
                }
            }
        }
        if (s == n_strips - 1) score = lane_value(cur, last_lane);       // the last step computed (rows - 1, cols - 1)
        plo = llo; phi = whi;
        __threadfence();
    }
    score = __uint_as_float(uniform32(__float_as_uint(score)));

    // traceback from (rows - 1, cols - 1).  lo / hi: the intervals of the 64 rows of strip held_s, one per lane
    const bool want_path = B.path != nullptr;
    const uint32_t cap = J.path_cap;
    uint2 *path = want_path ? reinterpret_cast<uint2 *>(B.path) + J.path_off : nullptr;
    uint32_t i = rows - 1, j = cols - 1, held_s = DTW_NONE_IDX, held_b = DTW_NONE_IDX, w = 0, lo = 1, hi = 0, wlo = 0;
    uint32_t pj = 0, pi = 0;
    uint64_t p = 0;
    bool left = false;
    for (;;) {
        const uint32_t s = i >> 6, l = i & 63u;
        if (s != held_s) {
            const uint32_t r = s * 64 + lane;
            lo = 1; hi = 0;
            if (r < rows) { lo = dtw_band_lo(r, rows, cols, W); hi = dtw_band_hi(r, rows, cols, W); }
            wlo = lane_value(lo, 0);
            held_s = s; held_b = DTW_NONE_IDX;
        }
        const uint32_t t = j - wlo + l, b = t >> 4;
        if (j < lane_value(lo, l) || j > lane_value(hi, l) || b >= n_blocks) { left = true; break; }     // no such cell: nothing stored
        if (lane == (uint32_t)(p & 63u)) { pj = j; pi = i; }
        ++p;
        if ((p & 63u) == 0) {
            const uint64_t at = p - 64 + lane;
            if (want_path && at < cap) path[at] = make_uint2(pj, pi);
        }
        if (i == 0 && j == 0) break;
        if (b != held_b) {
            w = crumbs[((uint64_t)s * n_blocks + b) * 64 + lane];
            held_b = b;
        }
        const uint32_t mv = (lane_value(w, l) >> (2u * (t & 15u))) & 3u;
        if (i == 0 || (mv == MOVE_H && j > 0)) --j;
        else if (j == 0 || mv == MOVE_V) --i;
        else { --i; --j; }
    }
    if ((p & 63u) != 0) {
        const uint64_t at = (p & ~(uint64_t)63) + lane;
        if (want_path && lane < (uint32_t)(p & 63u) && at < cap) path[at] = make_uint2(pj, pi);
    }
    dtw_write_result(B, J, score, p, left ? UNC_DTW_LEFT_BAND : want_path && p > cap ? UNC_DTW_PATH_TRUNCATED : UNC_DTW_OK);
}

template <int COST> __global__ void __launch_bounds__(64) k_dtw_band(DtwBatch B) {
    for (;;) {
        const uint32_t q = dtw_take_job(B);
        if (q >= B.n_jobs) return;
        const DtwJob J = B.jobs[q];
        dtw_band_one<COST>(B, J);
        wave_sync();
    }
}

}  // namespace
}  // namespace unc

// k_dtw_adapt, the band that follows the path, is compiled as part of this translation unit: it shares the cost and the leaves above
#include "k_dtw_adapt.hip"

namespace unc {

void launch_dtw(const DtwBatch &b, uint32_t cost, uint32_t grid, hipStream_t st) {
    switch (b.layout.kind) {
    case DtwKind::Adapt: launch_dtw_adapt(b, cost, grid, st); break;
    case DtwKind::Band:
        if (cost == UNC_DTW_R94D) hipLaunchKernelGGL(k_dtw_band<(int)UNC_DTW_R94D>, dim3(grid), dim3(64), 0, st, b);
        else hipLaunchKernelGGL(k_dtw_band<(int)UNC_DTW_R94P>, dim3(grid), dim3(64), 0, st, b);
        break;
    case DtwKind::Full:
        if (cost == UNC_DTW_R94D) hipLaunchKernelGGL(k_dtw<(int)UNC_DTW_R94D>, dim3(grid), dim3(64), 0, st, b);
        else hipLaunchKernelGGL(k_dtw<(int)UNC_DTW_R94P>, dim3(grid), dim3(64), 0, st, b);
        break;
    }
}

}  // namespace unc
