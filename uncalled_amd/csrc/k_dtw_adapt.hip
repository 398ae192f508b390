// k_dtw_adapt: DTW within a band of B rows that follows the path, with an open end (unc_dtw_adapt_batch, include/uncalled_hip.h).
// Compiled as part of k_dtw.hip's translation unit: the cost, the cell with its tie rule, the model's row, the result and the
// queue are the leaves at that file's top.
//
// One wavefront per alignment, swept by anti-diagonals d = i + j.  On d the band holds the rows [lo_d, lo_d + B); after d it moves one
// row down or stays (the next anti-diagonal then lies one column to the right), by the scores of its two end cells.  The B cells of an
// anti-diagonal are independent; lane l holds N = B / 64 of them in registers.  A cell's place does not slide with the band: row i
// lives in slot i mod B (lane slot / N, cell slot % N) for as long as the band holds it, and when the band moves down the slot of
// the row that left is taken by the row that enters.  So, whatever the band's last moves were,
//   H (i, j - 1) on d - 1 is the slot's own last value,
//   V (i - 1, j) on d - 1 is the last value of the slot before it: the lane's own previous cell, or the previous lane's last cell
//     (one wave_shr:1, lane 0 takes lane 63's),
//   D (i - 1, j - 1) on d - 2 is what V was one step ago,
// and what the moves decide is only whether such a slot held that row then: three compares against lo_{d-1} and lo_{d-2}.  A cell
// outside the matrix holds DTW_MAX_COST, the value an absent predecessor reads as.  The events move with V (the event of (i, j) on d
// was the event of (i - 1, j) on d - 1); a new event enters at the band's first row inside the matrix whenever that row stays, a new
// k-mer's model values enter at the band's last row whenever the band moves down, both from registers loaded 64 at a time.
// The two end scores are read with v_readlane, so the move, lo_d and every branch below are scalar.
//
// Memory (dtw_adapt_* of dtw_dev.h): per block of 16 anti-diagonals N words per lane (cell c of lane l: word (block * N + c) * 64 + l,
// its 16 moves at 2 bits each: coalesced 256-byte stores), then lo_d as int32, stored 64 anti-diagonals at a time.  The traceback runs
// on the same wavefront: it holds the words of the block and the 64 lo_d it is in, and writes the path 64 pairs at a time.

namespace unc {
namespace {

__device__ __forceinline__ int64_t max64(int64_t a, int64_t b) { return a > b ? a : b; }
__device__ __forceinline__ int64_t min64(int64_t a, int64_t b) { return a < b ? a : b; }

// the value of lane - 1, lane 0: of lane 63
__device__ __forceinline__ float rot_up(float v) {
    const uint32_t u = __float_as_uint(v);
    const uint32_t last = lane_value(u, 63u);
    const uint32_t s = dpp_mov32<0x138>(u);          // wave_shr:1 (lane 0 has no source)
    return __uint_as_float(lane_id() == 0 ? last : s);
}

// a[c] of the N (1, 2 or 4) values a lane holds, c wave-uniform.  (By value: an array handed over by reference is not split into
// registers before the compiler looks for arrays to move into LDS.)
template <class T> __device__ __forceinline__ T pick4(uint32_t c, T a0, T a1, T a2, T a3) {
    const T x = (c & 1u) ? a1 : a0, y = (c & 1u) ? a3 : a2;
    return (c & 2u) ? y : x;
}
#define UNC_PICK(a, c) pick4((c), a[0], a[N > 1 ? 1 : 0], a[N > 2 ? 2 : 0], a[N > 3 ? 3 : 0])

template <int COST, int N> __device__ void dtw_adapt_one(const DtwBatch &B, const DtwJob &J) {
    static_assert(N == 1 || N == 2 || N == 4, "cells per lane");
    constexpr uint32_t BW = 64u * N;
    const uint32_t lane = (uint32_t)lane_id();
    const uint32_t rows = uniform32(J.rows), cols = uniform32(J.cols);
    const uint32_t n_diag = rows + cols - 1;           // (both below 2^31)
    const float dw = B.dw, hw = B.hw, vw = B.vw;
    const float *ev = B.events + J.ev_off;
    const uint16_t *km = B.kmers + J.km_off;
    uint32_t *crumbs = B.crumbs + J.crumb_off;
    int32_t *los = reinterpret_cast<int32_t *>(crumbs + dtw_adapt_lo_first(rows, cols, BW));

    // the band of d = 0: rows [-B/2, B/2); slot s holds row s, or s - B from the band's middle on
    int32_t row[N];
    float cur[N], p2[N], e[N], mu[N], v2[N], ln[N];
    uint32_t cw[N];
#pragma unroll
    for (int c = 0; c < N; ++c) {
        const uint32_t s = lane * N + c;
        row[c] = s < BW / 2 ? (int32_t)s : (int32_t)s - (int32_t)BW;
        cur[c] = DTW_MAX_COST; p2[c] = DTW_MAX_COST; e[c] = 0.0f; cw[c] = 0;
        mu[c] = 0.0f; v2[c] = 1.0f; ln[c] = 0.0f;
        if (s < BW / 2 && s < rows) {
            const ModelRow r = model_row(B.model, km[s]);
            mu[c] = r.mu; v2[c] = r.v2; ln[c] = r.ln;
        }
    }
    float rot_prev = lane == 0 ? 0.0f : DTW_MAX_COST;       // D of (0, 0): the start
    float ev_reg = 0.0f, mu_reg = 0.0f, v2_reg = 1.0f, ln_reg = 0.0f;
    uint32_t km_held = DTW_NONE_IDX;        // the block of 64 k-mers whose model values mu_reg / v2_reg / ln_reg hold
    int32_t lo = -(int32_t)(BW / 2), lo1 = lo, lo2 = lo, lo_keep = 0;
    uint32_t jt = 0;                        // the next event to enter
    bool down = false;                      // the move that led to d
    // the open end: the first smallest score of column cols - 1 (a candidate compared smaller), and that column's last computed cell
    float best_v = INFINITY, last_v = 0.0f;
    uint32_t best_i = DTW_NONE_IDX, last_i = DTW_NONE_IDX;
    uint32_t d = 0;
    for (; d < n_diag; ++d) {
        // ---- the band of d
        lo = down ? lo1 + 1 : lo1;
        const int64_t top = lo > 0 ? lo : 0;
        const int64_t it = max64(top, (int64_t)d - (int64_t)(cols - 1));
        const int64_t ib = min64(min64((int64_t)lo + BW - 1, (int64_t)rows - 1), (int64_t)d);
        if (it > ib) break;                 // no cell of d is in the band and the matrix: the sweep ends
        // ---- what moves into the cells
        const float rot_c = rot_up(cur[N - 1]), rot_e = rot_up(e[N - 1]);
        float up[N], dg[N];
#pragma unroll
        for (int c = N - 1; c > 0; --c) { up[c] = cur[c - 1]; dg[c] = p2[c - 1]; e[c] = e[c - 1]; }
        up[0] = rot_c; dg[0] = rot_prev; e[0] = rot_e;
        rot_prev = rot_c;
        bool entered[N];
#pragma unroll
        for (int c = 0; c < N; ++c) entered[c] = false;
        if (down) {     // row lo1 left, row lo1 + B enters in its slot
            const uint32_t nb = (uint32_t)lo1 + BW;         // (lo1 + B < 2^31 + 256)
            if ((nb >> 6) != km_held && nb < rows) {
                const uint32_t r = (nb & ~63u) + lane;
                mu_reg = 0.0f; v2_reg = 1.0f; ln_reg = 0.0f;
                if (r < rows) {
                    const ModelRow m = model_row(B.model, km[r]);
                    mu_reg = m.mu; v2_reg = m.v2; ln_reg = m.ln;
                }
                km_held = nb >> 6;
            }
            const float m0 = lane_value(mu_reg, nb & 63u), m1 = lane_value(v2_reg, nb & 63u), m2 = lane_value(ln_reg, nb & 63u);
#pragma unroll
            for (int c = 0; c < N; ++c)
                if (row[c] == lo1) { row[c] = (int32_t)nb; mu[c] = m0; v2[c] = m1; ln[c] = m2; entered[c] = true; }
        }
        if (!down || lo <= 0) {     // the first row inside the matrix stayed: it is one column further
            if ((jt & 63u) == 0) {
                const uint32_t c = jt + lane;
                ev_reg = c < cols ? ev[c] : 0.0f;
            }
            const float e0 = lane_value(ev_reg, jt & 63u);
            ++jt;
#pragma unroll
            for (int c = 0; c < N; ++c)
                if (row[c] == (int32_t)top) e[c] = e0;
        }
        // ---- the cells
#pragma unroll
        for (int c = 0; c < N; ++c) {
            const int32_t i = row[c];
            const bool present = (uint32_t)i < rows && d - (uint32_t)i < cols;
            const float hp = entered[c] ? DTW_MAX_COST : cur[c];                                    // i was in the band of d - 1
            const float vp = i != lo1 ? up[c] : DTW_MAX_COST;                                       // i - 1 was
            const float dp = (uint32_t)(i - 1 - lo2) < BW ? dg[c] : DTW_MAX_COST;                   // i - 1 was in the band of d - 2
            const DtwCell x = dtw_cell(dp, hp, vp, dtw_cost<COST>(e[c], mu[c], v2[c], ln[c]), dw, hw, vw);
            p2[c] = cur[c];
            cur[c] = present ? x.m : DTW_MAX_COST;
            if (present) cw[c] |= x.mv << (2u * (d & 15u));
        }
        if ((d & 15u) == 15u) {
#pragma unroll
            for (int c = 0; c < N; ++c) {
                UNC_SIM_CHECK(((uint64_t)(d >> 4) * N + c) * 64 + lane < dtw_adapt_lo_first(rows, cols, BW));
                crumbs[((uint64_t)(d >> 4) * N + c) * 64 + lane] = cw[c];
                cw[c] = 0;
            }
        }
        if (lane == (d & 63u)) lo_keep = lo;
        if ((d & 63u) == 63u) {
            UNC_SIM_CHECK(dtw_adapt_lo_first(rows, cols, BW) + (d & ~63u) + lane < dtw_adapt_words(rows, cols, BW));
            los[(d & ~63u) + lane] = lo_keep;
        }
        // ---- the move, by the two end cells
        const uint32_t st = (uint32_t)it & (BW - 1), sb = (uint32_t)ib & (BW - 1);
        const float vt = lane_value(UNC_PICK(cur, st % N), st / N), vb = lane_value(UNC_PICK(cur, sb % N), sb / N);
        down = vb < vt ? true : vt < vb ? false : (d & 1u) != 0;
        if ((int64_t)lo + BW - 1 >= (int64_t)rows - 1) down = false;       // the band holds the last row already: it stays
        if (d >= cols - 1 && (uint64_t)it == (uint64_t)d - (cols - 1)) {       // (it, cols - 1) was computed
            last_v = vt; last_i = (uint32_t)it;
            if (vt < best_v) { best_v = vt; best_i = (uint32_t)it; }
        }
        lo2 = lo1; lo1 = lo;
    }
    const uint32_t n_done = d;              // anti-diagonals computed: [0, n_done)
    if ((n_done & 15u) != 0) {
#pragma unroll
        for (int c = 0; c < N; ++c) {
            UNC_SIM_CHECK(((uint64_t)(n_done >> 4) * N + c) * 64 + lane < dtw_adapt_lo_first(rows, cols, BW));
            crumbs[((uint64_t)(n_done >> 4) * N + c) * 64 + lane] = cw[c];
        }
    }
    if ((n_done & 63u) != 0 && lane < (n_done & 63u)) {
        UNC_SIM_CHECK(dtw_adapt_lo_first(rows, cols, BW) + (n_done & ~63u) + lane < dtw_adapt_words(rows, cols, BW));
        los[(n_done & ~63u) + lane] = lo_keep;
    }
    __threadfence();        // lanes read what other lanes wrote

    // ---- the end cell
    uint32_t ei = best_i != DTW_NONE_IDX ? best_i : last_i;
    float score = best_i != DTW_NONE_IDX ? best_v : last_v;
    const bool none = ei == DTW_NONE_IDX;   // no cell of the last column was computed
    if (none) score = 0.0f;
    ei = uniform32(ei);
    score = __uint_as_float(uniform32(__float_as_uint(score)));

    // ---- traceback, dtw.hpp:100-119, from (ei, cols - 1) to (0, 0)
    const bool want_path = B.path != nullptr;
    const uint32_t cap = J.path_cap;
    uint2 *path = want_path ? reinterpret_cast<uint2 *>(B.path) + J.path_off : nullptr;
    uint32_t i = ei, j = cols - 1, held_b = DTW_NONE_IDX, held_l = DTW_NONE_IDX;
    uint32_t w[N];
#pragma unroll
    for (int c = 0; c < N; ++c) w[c] = 0;
    int32_t lo_w = 0;
    uint32_t pj = 0, pi = 0;
    uint64_t p = 0;
    bool left = none;
    while (!left) {
        const uint32_t dd = i + j;
        if ((dd >> 6) != held_l) {
            // (dd < n_done: every cell the traceback is led to lies on an anti-diagonal below the end cell's)
            const uint32_t at = (dd & ~63u) + lane;
            lo_w = at < n_done ? los[at] : 0;
            held_l = dd >> 6;
        }
        const int32_t lod = (int32_t)lane_value((uint32_t)lo_w, dd & 63u);
        if ((uint32_t)((int32_t)i - lod) >= BW) { left = true; break; }        // never computed: nothing stored
        if (lane == (uint32_t)(p & 63u)) { pj = j; pi = i; }
        ++p;
        if ((p & 63u) == 0) {
            const uint64_t at = p - 64 + lane;
            if (want_path && at < cap) path[at] = make_uint2(pj, pi);
        }
        if (i == 0 && j == 0) break;
        if ((dd >> 4) != held_b) {
#pragma unroll
            for (int c = 0; c < N; ++c) w[c] = crumbs[((uint64_t)(dd >> 4) * N + c) * 64 + lane];
            held_b = dd >> 4;
        }
        const uint32_t s = i & (BW - 1);
        const uint32_t mv = (lane_value(UNC_PICK(w, s % N), s / N) >> (2u * (dd & 15u))) & 3u;
        if (i == 0 || (mv == MOVE_H && j > 0)) --j;
        else if (j == 0 || mv == MOVE_V) --i;
        else { --i; --j; }
    }
    if ((p & 63u) != 0) {
        const uint64_t at = (p & ~(uint64_t)63) + lane;
        if (want_path && lane < (uint32_t)(p & 63u) && at < cap) path[at] = make_uint2(pj, pi);
    }
    dtw_write_result(B, J, score, p,
                     left ? UNC_DTW_LEFT_BAND : want_path && p > cap ? UNC_DTW_PATH_TRUNCATED : ei == rows - 1 ? UNC_DTW_REF_END : UNC_DTW_OK);
}

#undef UNC_PICK

template <int COST, int N> __global__ void __launch_bounds__(64) k_dtw_adapt(DtwBatch B) {
    for (;;) {
        const uint32_t q = dtw_take_job(B);
        if (q >= B.n_jobs) return;
        const DtwJob J = B.jobs[q];
        dtw_adapt_one<COST, N>(B, J);
        wave_sync();
    }
}

template <int N> void launch_dtw_adapt_n(const DtwBatch &b, uint32_t cost, uint32_t grid, hipStream_t st) {
    if (cost == UNC_DTW_R94D) hipLaunchKernelGGL((k_dtw_adapt<(int)UNC_DTW_R94D, N>), dim3(grid), dim3(64), 0, st, b);
    else hipLaunchKernelGGL((k_dtw_adapt<(int)UNC_DTW_R94P, N>), dim3(grid), dim3(64), 0, st, b);
}

// b.layout.width: 64, 128 or 256 (dtw_adapt_band_ok, checked by the host)
void launch_dtw_adapt(const DtwBatch &b, uint32_t cost, uint32_t grid, hipStream_t st) {
    if (b.layout.width == 64) launch_dtw_adapt_n<1>(b, cost, grid, st);
    else if (b.layout.width == 128) launch_dtw_adapt_n<2>(b, cost, grid, st);
    else launch_dtw_adapt_n<4>(b, cost, grid, st);
}

}  // namespace
}  // namespace unc
