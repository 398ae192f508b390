// k_align_segments: an alignment's path in the read's sample coordinates -- one record per reference k-mer (row) on the path: the
// samples the k-mer spans and the current mean, deviation and normalised level over them (unc_segment_t, include/uncalled_hip.h).
// The reference prints DTW::get_path() (dtw.hpp:100-119, dtw_test.cpp:162-176) and stops there.
//
// A path is path_len pairs (column, row), end cell first; rows and columns both fall by at most one per pair.  So the rows on it
// are one contiguous run [row_first, row_first + n_rows), a row's pairs are one contiguous run of pair indices, and pair p is
// its row's HEAD (lowest column) iff p == path_len - 1 or row(p + 1) != row(p).  One wavefront takes one alignment of the round:
// its lanes stride over the pairs with 8-byte loads, 512 contiguous bytes a step, and a lane whose pair is a head walks the row's
// pairs towards lower p -- ascending column -- and writes the row's record.  A column c is the kept event col_evt[c] of the query
// (k_align_prep says which; with UNC_ALIGN_RAW the column is sample c itself).  No LDS, no atomics, no collectives: a row belongs
// to one lane.  The sums run in double in the order of the columns, one rounding per operation: the file is compiled with
// -ffp-contract=off, and every statement below is one operation.
#include <hip/hip_runtime.h>

#include <math.h>

#include "align_dev.h"
#include "dtw_dev.h"
#include "wave_prims.h"

namespace unc {
namespace {

constexpr uint32_t SEG_MAX_GRID = 1024;      // wavefronts of a launch: one for each SIMD of the MI355X; each takes every 1024th alignment

__global__ void __launch_bounds__(64) k_align_segments(SegArgs A) {
    const uint32_t lane = (uint32_t)lane_id();
    for (uint32_t a = blockIdx.x; a < A.n_jobs; a += gridDim.x) {
        const DtwJob J = A.jobs[a];
        const uint32_t q = J.out;
        const unc_dtw_result_t R = A.res[q];
        unc_seg_info_t inf;
        inf.row_first = 0; inf.n_rows = 0; inf.status = UNC_SEG_NONE; inf.pad = 0;
        // (the room on the device holds every pair, so the kernel's status is UNC_DTW_OK, UNC_DTW_REF_END: a whole path too, or
        // UNC_DTW_LEFT_BAND: a path without a start)
        if ((R.status != UNC_DTW_OK && R.status != UNC_DTW_REF_END) || R.path_len == 0 || R.path_len > (uint64_t)J.path_cap) {
            UNC_SIM_CHECK(R.path_len <= (uint64_t)J.path_cap);
            if (lane == 0) A.info[q] = inf;
            continue;
        }
        const uint32_t len = (uint32_t)R.path_len;
        const uint2 *path = reinterpret_cast<const uint2 *>(A.path) + J.path_off;       // x: column, y: row
        const AlignQuery Q = A.queries[q];
        const float scale = A.rec[q].scale, shift = A.rec[q].shift;
        const uint64_t smp0 = A.smp_st[q];
        const uint64_t room = A.seg_off[q + 1] - A.seg_off[q];
        unc_segment_t *seg = A.seg + A.seg_off[q];
        const uint32_t row_first = path[len - 1].y, n_rows = path[0].y - row_first + 1;
        UNC_SIM_CHECK(path[0].y < J.rows && row_first <= path[0].y);
        const unc_event_t *events = A.raw ? nullptr : A.events + Q.col_off;
        const uint32_t *col_evt = A.raw ? nullptr : A.col_evt + Q.col_off;
        const float *samples = A.means + Q.col_off;
        for (uint32_t p0 = 0; p0 < len; p0 += 64) {
            const uint32_t p = p0 + lane;
            if (p >= len) break;                      // (no collectives)
            const uint2 head = path[p];
            uint2 prev = make_uint2(0xFFFFFFFFu, 0xFFFFFFFFu);       // the pair before the head on the way from the start: the previous row's last
            if (p + 1 < len) prev = path[p + 1];
            if (prev.y == head.y) continue;           // not a head
            const uint32_t s = head.y - row_first;
            if ((uint64_t)s >= room || s >= n_rows) continue;
            double S = 0.0, QQ = 0.0;
            uint32_t N = 0, n_cols = 0, first_start = 0, last_end = 0;
            for (uint32_t k = p;; --k) {              // ascending column
                const uint2 pr = k == p ? head : path[k];
                if (pr.y != head.y) break;
                const uint32_t c = pr.x;
                UNC_SIM_CHECK(c < J.cols && c < Q.col_cap);
                if (c >= Q.col_cap) break;            // (cannot happen: the path's columns are the job's)
                unc_event_t e;
                if (A.raw) { e.mean = samples[c]; e.stdv = 0.0f; e.start = c; e.length = 1; }
                else {
                    const uint32_t ei = col_evt[c];
                    UNC_SIM_CHECK(ei < Q.col_cap);
                    if (ei >= Q.col_cap) break;
                    e = events[ei];
                }
                const double m = (double)e.mean, d = (double)e.stdv, l = (double)e.length;
                const double ml = m * l;
                S = S + ml;
                const double dd = d * d;
                const double mm = m * m;
                const double dm = dd + mm;
                const double ldm = l * dm;
                QQ = QQ + ldm;
                N += e.length;
                if (n_cols == 0) first_start = e.start;
                last_end = e.start + e.length;
                ++n_cols;
                if (k == 0) break;
            }
            const double n = (double)N;
            const double M = S / n;
            const double qn = QQ / n;
            const double m2 = M * M;
            const double var = qn - m2;
            unc_segment_t r;
            r.smp_st = smp0 + first_start;
            r.smp_span = last_end - first_start;
            r.smp_n = N;
            r.col_first = head.x;
            r.n_cols = n_cols;
            r.mean = (float)M;
            r.stdv = (float)sqrt(fmax(var, 0.0));
            r.level = __fadd_rn(__fmul_rn(scale, r.mean), shift);        // Normalizer::at, normalizer.cpp:114-118
            r.shared = prev.x == head.x ? 1u : 0u;
            seg[s] = r;
        }
        if (lane == 0) {
            inf.row_first = row_first; inf.n_rows = n_rows;
            inf.status = (uint64_t)n_rows > room ? UNC_SEG_TRUNCATED : UNC_SEG_OK;
            A.info[q] = inf;
        }
    }
}

}  // namespace

void launch_align_segments(const SegArgs &a, hipStream_t st) {
    const uint32_t grid = a.n_jobs < SEG_MAX_GRID ? a.n_jobs : SEG_MAX_GRID;
    hipLaunchKernelGGL(k_align_segments, dim3(grid), dim3(64), 0, st, a);
}

}  // namespace unc
