// Host side of unc_align_batch (include/uncalled_hip.h): argument checks, the layout of the queries' slices, means and levels in
// device memory, the launches of the stages (k_align.hip, k_events.hip) and the hand-over to the DTW's planner (unc_dtw.cpp).
// Host copies that remain: the reads' samples in (unless on_device), the queries and k-mers in, one 32-byte record per query out
// between normalisation and DTW (the planner lays out back-pointers by column counts), results and paths out, levels out on request.
#include <hip/hip_runtime.h>

#include <math.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "align_dev.h"
#include "dtw_dev.h"
#include "unc_host_util.h"
#include "unc_kernels.h"

using namespace unc;

static thread_local float g_align_ms[4] = {0, 0, 0, 0};

extern "C" int unc_align_last_timing(float *ms4) {
    if (!ms4) return fail(UNC_ERR_ARG, "unc_align_last_timing: null argument");
    memcpy(ms4, g_align_ms, sizeof g_align_ms);
    return UNC_OK;
}

// PoreModel(vector, cmpl=false): model_mean_ is the float sum of the means in table order over the count (pore_model.hpp:82-99),
// init_stdv (:48-56) a float accumulator of double squares of float differences
extern "C" void unc_align_model_target(float *mean, float *stdv) {
    const float *mu = dtw_model_host();
    float s = 0;
    for (uint32_t k = 0; k < (uint32_t)UNC_NKMER; ++k) s = s + mu[k];
    s = s / (float)UNC_NKMER;
    float acc = 0;
    for (uint32_t k = 0; k < (uint32_t)UNC_NKMER; ++k) {
        const float d = mu[k] - s;
        acc = (float)((double)acc + (double)d * (double)d);
    }
    if (mean) *mean = s;
    if (stdv) *stdv = sqrtf(acc / (float)UNC_NKMER);
}

namespace {
struct HipEvents {       // (timing only)
    hipEvent_t e[4] = {nullptr, nullptr, nullptr, nullptr};
    ~HipEvents() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); }
};
}  // namespace

// The pipeline, from the arguments' checks to the results.  The queries' rows are `rows`' business (align_dev.h).
int unc::align_run(const char *who, int device, const unc_params_t *params, const unc_align_opts_t *opts, uint32_t n_reads, const int16_t *raw,
                   const uint64_t *offsets, const unc_calib_t *calib, int on_device, uint32_t n_queries, const unc_align_query_t *queries,
                   AlignRows &rows, uint64_t workspace_bytes, unc_align_result_t *results, float *levels, const uint64_t *lev_off,
                   uint32_t *path, const uint64_t *path_off, void *stream) {
    // ---- arguments: everything is checked before the device is touched
    if (!raw || !offsets || !calib || !queries || !results) return fail(UNC_ERR_ARG, "%s: null argument", who);
    if (path && !path_off) return fail(UNC_ERR_ARG, "%s: path without path_off", who);
    if (levels && !lev_off) return fail(UNC_ERR_ARG, "%s: levels without lev_off", who);
    if (device < 0 || device >= DTW_MAX_DEVICES) return fail(UNC_ERR_ARG, "%s: device %d", who, device);
    unc_align_opts_t O;
    memset(&O, 0, sizeof O);
    if (opts) O = *opts;
    if (O.flags & ~(UNC_ALIGN_DTW_PARAMS | UNC_ALIGN_NO_MASK | UNC_ALIGN_RAW | UNC_ALIGN_TARGET_MODEL))
        return fail(UNC_ERR_ARG, "%s: unknown flags %#x", who, O.flags);
    unc_dtw_params_t prm = {UNC_DTW_NONE, UNC_DTW_R94D, 1.0f, 1.0f, 1.0f};        // dtw_test.cpp:76-78,162
    if (O.flags & UNC_ALIGN_DTW_PARAMS) prm = O.dtw;
    if (prm.subseq > UNC_DTW_COL) return fail(UNC_ERR_ARG, "%s: unknown subseq %u", who, prm.subseq);
    if (prm.cost > UNC_DTW_R94D) return fail(UNC_ERR_ARG, "%s: unknown cost %u", who, prm.cost);
    if (O.band && prm.subseq != UNC_DTW_NONE) return fail(UNC_ERR_ARG, "%s: the band is global only (subseq %u)", who, prm.subseq);
    unc_params_t P;
    if (params) P = *params;
    else unc_params_default(&P);
    if (P.window_length1 != UNC_WINDOW1 || P.window_length2 != UNC_WINDOW2)
        return fail(UNC_ERR_ARG, "%s: the event detector's windows must be %d and %d", who, UNC_WINDOW1, UNC_WINDOW2);
    memset(g_align_ms, 0, sizeof g_align_ms);
    if (n_queries == 0) return UNC_OK;
    for (uint32_t i = 0; i < n_reads; ++i)
        if (offsets[i + 1] < offsets[i]) return fail(UNC_ERR_ARG, "%s: offsets must ascend", who);
    const bool raw_mode = (O.flags & UNC_ALIGN_RAW) != 0;
    std::vector<AlignQuery> hq(n_queries);
    uint64_t n_gather = 0, n_cols = 0;
    for (uint32_t q = 0; q < n_queries; ++q) {
        const unc_align_query_t &u = queries[q];
        if (u.read >= n_reads) return fail(UNC_ERR_ARG, "%s: query %u names read %u of %u", who, q, u.read, n_reads);
        const uint64_t len = offsets[u.read + 1] - offsets[u.read];
        const uint64_t en = u.smp_en == 0 ? len : u.smp_en;            // dtw_test.cpp:123-132
        if (u.smp_en != 0 && u.smp_st > u.smp_en) return fail(UNC_ERR_ARG, "%s: query %u: smp_st %llu > smp_en %llu", who, q,
                                                              (unsigned long long)u.smp_st, (unsigned long long)u.smp_en);
        if (en > len || u.smp_st > len) return fail(UNC_ERR_ARG, "%s: query %u: [%llu, %llu) is not inside the read's %llu samples", who, q,
                                                    (unsigned long long)u.smp_st, (unsigned long long)en, (unsigned long long)len);
        if (en - u.smp_st >= (1ull << 31)) return fail(UNC_ERR_ARG, "%s: query %u: 2^31 or more samples", who, q);
        uint64_t km_at = 0;
        uint32_t km_n = 0;
        if (int rc = rows.rows(q, &km_at, &km_n)) return rc;
        if (path && path_off[q + 1] < path_off[q]) return fail(UNC_ERR_ARG, "%s: path_off must ascend", who);
        if (levels && lev_off[q + 1] < lev_off[q]) return fail(UNC_ERR_ARG, "%s: lev_off must ascend", who);
        AlignQuery &a = hq[q];
        memset(&a, 0, sizeof a);
        a.src_off = offsets[u.read] - offsets[0] + u.smp_st;
        a.n_smp = (uint32_t)(en - u.smp_st);
        a.dst_off = n_gather;
        a.col_off = n_cols;
        a.km_off = km_at;
        a.n_km = km_n;
        // (peak_detect emits a peak once it lies more than window_length / 2 samples back and then starts afresh: the short detector
        // fires at most every third sample, the long one every fifth.  An event that finds its room full is reported below)
        a.col_cap = raw_mode ? a.n_smp : a.n_smp / 2 + 16;
        a.calib = calib[u.read];
        n_gather += a.n_smp;
        n_cols += a.col_cap;
    }
    if (int rc = rows.check()) return rc;

    // ---- device
    HIPCHK(hipSetDevice(device));
    hipStream_t st = (hipStream_t)stream;
    const float *d_model = nullptr;
    if (int rc = dtw_model_device(device, &d_model)) return rc;
    DevBuf<int16_t> d_raw_own, d_gather;
    DevBuf<float> d_means, d_levels;
    const uint16_t *d_kmers = nullptr;
    DevBuf<AlignQuery> d_q;
    DevBuf<AlignRecord> d_rec;
    DevBuf<uint64_t> d_goff, d_moff;
    DevBuf<unc_calib_t> d_calib;
    DevBuf<unc_evt_info_t> d_info;
    const int16_t *d_raw = raw + offsets[0];
    if (!on_device) {
        const uint64_t n_smp = offsets[n_reads] - offsets[0];
        HIPCHK(d_raw_own.alloc(n_smp));
        HIPCHK(hipMemcpyAsync(d_raw_own.p, raw + offsets[0], n_smp * sizeof(int16_t), hipMemcpyHostToDevice, st));
        d_raw = d_raw_own.p;
    }
    HIPCHK(d_q.alloc(n_queries)); HIPCHK(d_rec.alloc(n_queries));
    HIPCHK(d_means.alloc(n_cols)); HIPCHK(d_levels.alloc(n_cols));
    HIPCHK(hipMemcpyAsync(d_q.p, hq.data(), (size_t)n_queries * sizeof(AlignQuery), hipMemcpyHostToDevice, st));
    if (int rc = rows.queue(st, &d_kmers)) return rc;
    std::vector<uint64_t> goff, moff;
    std::vector<unc_calib_t> qcal;
    DevReads rd{};
    if (!raw_mode) {       // every slice is a read of its own to k_events
        HIPCHK(d_gather.alloc(n_gather, 64));
        goff.resize((size_t)n_queries + 1); moff.resize((size_t)n_queries + 1); qcal.resize(n_queries);
        for (uint32_t q = 0; q < n_queries; ++q) { goff[q] = hq[q].dst_off; moff[q] = hq[q].col_off; qcal[q] = hq[q].calib; }
        goff[n_queries] = n_gather; moff[n_queries] = n_cols;
        HIPCHK(d_goff.alloc((size_t)n_queries + 1)); HIPCHK(d_moff.alloc((size_t)n_queries + 1)); HIPCHK(d_calib.alloc(n_queries));
        HIPCHK(d_info.alloc(n_queries));
        HIPCHK(hipMemcpyAsync(d_goff.p, goff.data(), goff.size() * 8, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(d_moff.p, moff.data(), moff.size() * 8, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(d_calib.p, qcal.data(), qcal.size() * sizeof(unc_calib_t), hipMemcpyHostToDevice, st));
        rd.raw = d_gather.p; rd.offsets = d_goff.p; rd.calib = d_calib.p; rd.means = d_means.p; rd.moff = d_moff.p; rd.info = d_info.p;
        rd.n_reads = n_queries;
        unc_align_model_target(&rd.tgt_mean, &rd.tgt_stdv);       // (k_events' own scale and shift are not used here)
    }
    HipEvents ev;       // (all allocations and uploads are queued above, so that the spans between the events hold kernels only)
    for (hipEvent_t &x : ev.e) HIPCHK(hipEventCreate(&x));

    // a. the slices, then event detection on each
    HIPCHK(hipEventRecord(ev.e[0], st));
    launch_align_gather(d_raw, d_q.p, n_queries, raw_mode ? nullptr : d_gather.p, raw_mode ? d_means.p : nullptr, st);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(ev.e[1], st));
    if (!raw_mode) {
        // as few slices per wavefront as a grid of 2048 wavefronts allows (the kernel is sequential per slice)
        const uint32_t rpw = std::min<uint32_t>(64u, std::max<uint32_t>(1u, (n_queries + 2047u) / 2048u));
        launch_events(rd, P, st, rpw);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipEventRecord(ev.e[2], st));

    // b. - d. mask, target, normalisation
    AlignPrep ap{};
    ap.queries = d_q.p; ap.n_queries = n_queries; ap.flags = O.flags;
    ap.info = raw_mode ? nullptr : d_info.p;
    ap.means = d_means.p;
    ap.levels = d_levels.p;
    ap.kmers = d_kmers; ap.model = d_model;
    unc_align_model_target(&ap.model_mean, &ap.model_stdv);
    ap.rec = d_rec.p;
    launch_align_prep(ap, st);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(ev.e[3], st));
    std::vector<AlignRecord> rec(n_queries);
    std::vector<unc_evt_info_t> info(raw_mode ? 0 : n_queries);
    HIPCHK(hipMemcpyAsync(rec.data(), d_rec.p, (size_t)n_queries * sizeof(AlignRecord), hipMemcpyDeviceToHost, st));
    if (!raw_mode) HIPCHK(hipMemcpyAsync(info.data(), d_info.p, (size_t)n_queries * sizeof(unc_evt_info_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    for (int i = 0; i < 3; ++i) HIPCHK(hipEventElapsedTime(&g_align_ms[i], ev.e[i], ev.e[i + 1]));
    for (uint32_t q = 0; q < n_queries && !raw_mode; ++q)
        if (info[q].pad) return fail(UNC_ERR_OVERFLOW, "%s: query %u has more events than its room of %u", who, q, hq[q].col_cap);

    // e. the DTW over the levels where they lie
    std::vector<DtwJob> jobs(n_queries);
    std::vector<uint8_t> skip(n_queries, 0);
    std::vector<unc_dtw_result_t> dres(n_queries);
    memset(dres.data(), 0, dres.size() * sizeof(unc_dtw_result_t));
    for (uint32_t q = 0; q < n_queries; ++q) {
        unc_align_result_t &r = results[q];
        memset(&r, 0, sizeof r);
        r.n_events = rec[q].n_events; r.n_kept = rec[q].n_kept;
        r.tgt_mean = rec[q].tgt_mean; r.tgt_stdv = rec[q].tgt_stdv; r.scale = rec[q].scale; r.shift = rec[q].shift;
        if (r.n_kept == 0) { r.status = UNC_ALIGN_NO_COLUMNS; skip[q] = 1; }
        else if (O.max_events && r.n_kept > O.max_events) { r.status = UNC_ALIGN_TOO_MANY; skip[q] = 1; }
        DtwJob &j = jobs[q];
        memset(&j, 0, sizeof j);
        j.ev_off = hq[q].col_off; j.km_off = hq[q].km_off;
        j.rows = hq[q].n_km; j.cols = r.n_kept;
        j.out = q;
        const uint64_t room = path ? path_off[q + 1] - path_off[q] : 0;
        j.path_cap = skip[q] ? 0 : (uint32_t)std::min<uint64_t>(room, (uint64_t)j.rows + j.cols - 1);
    }
    if (int rc = dtw_run_device(device, n_queries, d_levels.p, d_kmers, jobs.data(), skip.data(), &prm, O.band, workspace_bytes, dres.data(),
                                path, path_off, st))
        return rc;
    (void)unc_dtw_last_timing(&g_align_ms[3], nullptr, nullptr);
    for (uint32_t q = 0; q < n_queries; ++q) {
        if (skip[q]) continue;
        results[q].dtw = dres[q];
        results[q].status = dres[q].status;
    }
    if (levels) {       // the tap: one copy of all levels, dealt out on the host
        std::vector<float> h((size_t)n_cols);
        HIPCHK(hipMemcpyAsync(h.data(), d_levels.p, (size_t)n_cols * sizeof(float), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        for (uint32_t q = 0; q < n_queries; ++q) {
            const uint64_t got = std::min<uint64_t>(results[q].n_kept, lev_off[q + 1] - lev_off[q]);
            memcpy(levels + lev_off[q], h.data() + hq[q].col_off, got * sizeof(float));
        }
    }
    return UNC_OK;
}

// ------------------------------------------------------------------ unc_align_batch: the caller's k-mers, uploaded
namespace {
struct UploadedRows : AlignRows {
    const uint16_t *kmers;
    const uint64_t *km_off;
    uint32_t n_queries;
    DevBuf<uint16_t> d_kmers;
    UploadedRows(const uint16_t *k, const uint64_t *off, uint32_t n) : kmers(k), km_off(off), n_queries(n) {}
    int rows(uint32_t q, uint64_t *at, uint32_t *n) override {
        if (km_off[q + 1] <= km_off[q]) return fail(UNC_ERR_ARG, "unc_align_batch: query %u has no k-mers", q);
        if (q && km_off[q] < km_off[q - 1]) return fail(UNC_ERR_ARG, "unc_align_batch: km_off must ascend");
        if (km_off[q + 1] - km_off[q] >= (1ull << 31)) return fail(UNC_ERR_ARG, "unc_align_batch: query %u: 2^31 or more k-mers", q);
        *at = km_off[q] - km_off[0];
        *n = (uint32_t)(km_off[q + 1] - km_off[q]);
        return UNC_OK;
    }
    int check() override {
        const uint64_t n_km = km_off[n_queries] - km_off[0];
        for (uint64_t i = 0; i < n_km; ++i)
            if (kmers[km_off[0] + i] >= UNC_NKMER) return fail(UNC_ERR_ARG, "unc_align_batch: k-mer %u at %llu is not below %d", kmers[km_off[0] + i],
                                                               (unsigned long long)(km_off[0] + i), UNC_NKMER);
        return UNC_OK;
    }
    int queue(hipStream_t st, const uint16_t **out) override {
        const uint64_t n_km = km_off[n_queries] - km_off[0];
        HIPCHK(d_kmers.alloc(n_km));
        HIPCHK(hipMemcpyAsync(d_kmers.p, kmers + km_off[0], n_km * sizeof(uint16_t), hipMemcpyHostToDevice, st));
        *out = d_kmers.p;
        return UNC_OK;
    }
};
}  // namespace

extern "C" int unc_align_batch(int device, const unc_params_t *params, const unc_align_opts_t *opts, uint32_t n_reads, const int16_t *raw,
                               const uint64_t *offsets, const unc_calib_t *calib, int on_device, uint32_t n_queries,
                               const unc_align_query_t *queries, const uint16_t *kmers, const uint64_t *km_off, uint64_t workspace_bytes,
                               unc_align_result_t *results, float *levels, const uint64_t *lev_off, uint32_t *path, const uint64_t *path_off,
                               void *stream) {
    if (!raw || !offsets || !calib || !queries || !kmers || !km_off || !results) return fail(UNC_ERR_ARG, "unc_align_batch: null argument");
    UploadedRows rows(kmers, km_off, n_queries);
    return align_run("unc_align_batch", device, params, opts, n_reads, raw, offsets, calib, on_device, n_queries, queries, rows, workspace_bytes,
                     results, levels, lev_off, path, path_off, stream);
}

// unc_align_ref_batch and the packed reference: unc_refseq.cpp and k_refseq.hip are compiled as part of this translation unit, so that
// every build of the alignment sources holds them
#include "unc_refseq.cpp"
