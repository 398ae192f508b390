// The stages of read-to-reference alignment between event detection (k_events.hip) and the DTW (k_dtw.hip), for a batch of queries
// (src/dtw_test.cpp:94-162):
//   k_align_gather   the queries' sample ranges, copied one after the other: k_events then takes every slice as a read of its own,
//                    with the detector reset at the slice's first sample (EventDetector::get_events, event_detector.cpp:114-126).
//                    k_events already walks sample by sample up to the first 16-byte boundary of a read, so a slice may start at
//                    any sample of its read and lie at any sample among the gathered ones.  With create_events off the kernel
//                    writes the calibrated samples instead (read_buffer.cpp:239-241), and they are the columns.
//   k_align_prep     EventProfiler::get_full_mask (event_profiler.hpp:71-104,129-151), the target of dtw_test.cpp:106-116,
//                    Normalizer::set_signal and pop (normalizer.cpp:31-44,114-128).  The levels go where k_dtw reads its columns.
//                    On request it also says which kept event became which column (col_evt), for k_align_segments (k_segments.hip).
// What is sequential and why.  The profiler's window is a Normalizer ring of 25 means: Welford's update until it is full, then the
// rolling update, both recurrences in double whose every step rounds; the decision for event n needs the window's state after
// event n + 24.  The target is a float running sum over the k-mers, the normaliser's two sums are double running sums over the
// kept means.  Any other order of the additions rounds differently, and the levels are compared with the reference bit for bit: one
// lane follows one query from its first event to its last level, and a wavefront carries as few queries as the batch allows.
// The window's ring itself is not kept: the mean that leaves the window when event n enters is event n - 25 of the query's means.
// All float expressions are written one IEEE operation at a time and the file is compiled with -ffp-contract=off.
#include <hip/hip_runtime.h>

#include <math.h>

#include "align_dev.h"
#include "wave_prims.h"

namespace unc {
namespace {

constexpr uint32_t PROF_LEN = 25;            // EventProfiler::PRMS_DEF.win_len, event_profiler.cpp:4-10
constexpr uint32_t PROF_MID = PROF_LEN / 2;  // WIN_MID
constexpr float PROF_STDV_MIN = 5.0f;        // win_stdv_min

__global__ void __launch_bounds__(256) k_align_gather(const int16_t *raw, const AlignQuery *queries, uint32_t n_queries, int16_t *gathered,
                                                      float *calibrated) {
    const uint32_t q = blockIdx.x;
    if (q >= n_queries) return;
    const AlignQuery Q = queries[q];
    const int16_t *src = raw + Q.src_off;
    if (calibrated) {
        UNC_SIM_CHECK(Q.n_smp <= Q.col_cap);
        float *dst = calibrated + Q.col_off;
        for (uint32_t i = threadIdx.x; i < Q.n_smp; i += blockDim.x)      // u16 reinterpretation of the stored i16, three float roundings
            dst[i] = __fdiv_rn(__fmul_rn(Q.calib.range, __fadd_rn((float)(int)(uint16_t)src[i], Q.calib.offset)), Q.calib.digitisation);
    } else {
        int16_t *dst = gathered + Q.dst_off;
        for (uint32_t i = threadIdx.x; i < Q.n_smp; i += blockDim.x) dst[i] = src[i];
    }
}

// EventProfiler::get_full_mask over means[0 .. n): the kept means, in order, to out[0 ..); returns how many.  col_evt (may be null):
// which event each of them is
__device__ __forceinline__ uint32_t stall_mask(const float *means, uint32_t n, float *out, uint32_t *col_evt) {
    double mean = 0.0, varsum = 0.0;                 // window_: Normalizer::reset
    uint32_t wn = 0, rd = 0, wr = 0, full = 0;
    uint32_t to_mask = 0, is_full = 0;
    uint32_t decided = 0, kept = 0;                  // mask.size(), and how many of them are true
    for (uint32_t e = 0; e < n; ++e) {
        const float x = means[e];
        // window_.push, normalizer.cpp:46-75 (never refused: a full window is popped below before the next event)
        if (wn == PROF_LEN) {
            const double oldevt = (double)means[e - PROF_LEN];
            const double oldmean = mean;
            mean += ((double)x - oldevt) / (double)PROF_LEN;
            varsum += ((double)x + oldevt - oldmean - mean) * ((double)x - oldevt);
        } else {
            wn++;
            const double dt1 = (double)x - mean;
            mean += dt1 / (double)wn;
            const double dt2 = (double)x - mean;
            varsum += dt1 * dt2;
        }
        wr = wr + 1 == PROF_LEN ? 0 : wr + 1;
        full = wr == rd ? 1u : 0u;
        const uint32_t unread = rd < wr ? wr - rd : (wn - rd) + wr;       // Normalizer::unread_size
        if (unread > PROF_MID) {
            const float win_stdv = (float)sqrt(varsum / (double)wn);      // Normalizer::get_stdv
            if (win_stdv < PROF_STDV_MIN) to_mask = PROF_LEN - 1;
            else if (to_mask > 0) to_mask--;
            if (full) {                                                   // events_.pop_front(), window_.pop()
                rd = rd + 1 == PROF_LEN ? 0 : rd + 1;
                full = 0;
                is_full = 1;
            }
        }
        if (is_full) {
            if (to_mask == 0) {
                if (col_evt) col_evt[kept] = decided;
                out[kept++] = means[decided];
            }
            decided++;
        }
    }
    for (; decided < n; ++decided) {                 // the tail loop, event_profiler.hpp:141-148
        if (to_mask == 0) {
            if (col_evt) col_evt[kept] = decided;
            out[kept++] = means[decided];
        } else to_mask--;
    }
    return kept;
}

__global__ void __launch_bounds__(64) k_align_prep(AlignPrep A, uint32_t queries_per_wave) {
    const uint32_t lane = (uint32_t)lane_id();
    const uint32_t q = blockIdx.x * queries_per_wave + lane;
    if (lane >= queries_per_wave || q >= A.n_queries) return;       // no collectives in this kernel
    const AlignQuery Q = A.queries[q];
    const bool raw_mode = (A.flags & UNC_ALIGN_RAW) != 0;
    const uint32_t n = raw_mode ? Q.n_smp : A.info[q].n_events;
    UNC_SIM_CHECK(n <= Q.col_cap);
    const float *means = A.means + Q.col_off;
    float *lev = A.levels + Q.col_off;

    // ---- b. the stall mask
    const float *src = means;
    uint32_t m = n;
    if (!raw_mode && !(A.flags & UNC_ALIGN_NO_MASK)) {
        m = stall_mask(means, n, lev, A.col_evt ? A.col_evt + Q.col_off : nullptr);
        src = lev;
    } else if (A.col_evt && !raw_mode) {
        for (uint32_t i = 0; i < n; ++i) A.col_evt[Q.col_off + i] = i;       // every event is a column
    }

    // ---- c. the target, dtw_test.cpp:106-116: `read_mean += get_mean(k)` is a float sum and `/= kmers.size()` a float division;
    // `pow(get_mean(k) - read_mean, 2)` is a float difference squared in double and added to the float accumulator in double
    float tgt_mean = A.model_mean, tgt_stdv = A.model_stdv;
    if (!(A.flags & UNC_ALIGN_TARGET_MODEL)) {
        const uint16_t *km = A.kmers + Q.km_off;
        float s = 0.0f;
        for (uint32_t i = 0; i < Q.n_km; ++i) s = __fadd_rn(s, A.model[km[i]]);
        s = __fdiv_rn(s, (float)Q.n_km);
        float v = 0.0f;
        for (uint32_t i = 0; i < Q.n_km; ++i) {
            const double d = (double)__fsub_rn(A.model[km[i]], s);
            v = (float)((double)v + d * d);
        }
        tgt_mean = s;
        tgt_stdv = sqrtf(__fdiv_rn(v, (float)Q.n_km));       // (sqrtf: correctly rounded, see k_events.hip)
    }

    // ---- d. Normalizer::set_signal, then at() for every column
    float scale = 0.0f, shift = 0.0f;
    if (m > 0) {
        double mean = 0.0;
        for (uint32_t i = 0; i < m; ++i) mean += (double)src[i];
        mean /= (double)m;
        double varsum = 0.0;
        for (uint32_t i = 0; i < m; ++i) {
            const double e = (double)src[i] - mean;
            varsum += e * e;
        }
        scale = (float)((double)tgt_stdv / sqrt(varsum / (double)m));
        shift = (float)((double)tgt_mean - (double)scale * mean);
        for (uint32_t i = 0; i < m; ++i) lev[i] = __fadd_rn(__fmul_rn(scale, src[i]), shift);
    }
    AlignRecord r;
    r.n_events = n; r.n_kept = m;
    r.tgt_mean = tgt_mean; r.tgt_stdv = tgt_stdv; r.scale = scale; r.shift = shift;
    r.pad[0] = 0; r.pad[1] = 0;
    A.rec[q] = r;
}

}  // namespace

void launch_align_gather(const int16_t *raw, const AlignQuery *queries, uint32_t n_queries, int16_t *gathered, float *calibrated, hipStream_t st) {
    hipLaunchKernelGGL(k_align_gather, dim3(n_queries), dim3(256), 0, st, raw, queries, n_queries, gathered, calibrated);
}

void launch_align_prep(const AlignPrep &p, hipStream_t st) {
    // as few queries per wavefront as a grid of 1024 wavefronts allows: the lanes of a wavefront wait for its longest query, but the
    // kernel is bound by instruction issue (one lane's f64 divisions and square roots), so a second wavefront on a SIMD only takes
    // turns with the first, while a second lane in a wavefront is free.  1024 = one wavefront for each SIMD of the MI355X
    uint32_t qpw = (p.n_queries + 1023u) / 1024u;
    if (qpw < 1u) qpw = 1u;
    if (qpw > 64u) qpw = 64u;
    hipLaunchKernelGGL(k_align_prep, dim3((p.n_queries + qpw - 1) / qpw), dim3(64), 0, st, p, qpw);
}

}  // namespace unc

// k_ref_kmers, which makes a batch's rows from the packed reference, is compiled as part of this translation unit, so that every
// build of the alignment sources holds it
#include "k_refseq.hip"
// and so is k_align_segments, which collapses a round's paths to one record per k-mer
#include "k_segments.hip"
// and k_model_accum, which sums a round's records per k-mer into a training accumulator
#include "k_model.hip"
// and k_pileup_accum with the covered-bin kernels, which sum a round's records per reference position into a pile-up
#include "k_pileup.hip"
// and the pile-up's level histograms with k_pileup_ks, the two-sample Kolmogorov-Smirnov distance of two of them
#include "k_pileup_hist.hip"
