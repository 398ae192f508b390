// Host side of unc_align_batch (include/uncalled_hip.h).  An entry point fills an AlignCall (align_dev.h) from its parameters;
// align_run is the list of steps over one AlignRun: argument checks, the layout of the queries' slices, means and levels in device
// memory, the launches of the stages (k_align.hip, k_events.hip), the hand-over to the DTW's planner (unc_dtw.cpp), the outputs.
// Host copies that remain: the reads' samples in (unless on_device), the queries and k-mers in, one 32-byte record per query out
// between normalisation and DTW (the planner lays out back-pointers by column counts), results and paths out, levels out on request.
#include <hip/hip_runtime.h>

#include <math.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "align_dev.h"
#include "dtw_dev.h"
#include "model_dev.h"
#include "pileup_dev.h"
#include "unc_host_util.h"
#include "unc_kernels.h"
#include "unc_model.h"

using namespace unc;

static thread_local float g_align_ms[4] = {0, 0, 0, 0};
static thread_local float g_seg_ms = 0;

extern "C" int unc_align_segments_last_timing(float *ms) {
    if (!ms) return fail(UNC_ERR_ARG, "unc_align_segments_last_timing: null argument");
    *ms = g_seg_ms;
    return UNC_OK;
}

extern "C" int unc_align_last_timing(float *ms4) {
    if (!ms4) return fail(UNC_ERR_ARG, "unc_align_last_timing: null argument");
    memcpy(ms4, g_align_ms, sizeof g_align_ms);
    return UNC_OK;
}

// PoreModel::get_means_mean / get_means_stdv of the template model, not complemented (the one builder, unc_model.h)
extern "C" void unc_align_model_target(float *mean, float *stdv) {
    const ModelTables &t = dtw_model_default();
    if (mean) *mean = t.mean;
    if (stdv) *stdv = t.stdv;
}

namespace unc {
// unc_model_acc.cpp (included below): what the alignment needs of an accumulator
void model_acc_set_timing(float ms);
int model_acc_device(const unc_model_acc *acc);
void model_acc_args(unc_model_acc *acc, ModelAccum *a);
// unc_pileup.cpp (included below): what the alignment needs of a pile-up
void pileup_set_timing(float ms);
int pileup_device(const unc_pileup *pu);
const unc_refseq *pileup_refseq(const unc_pileup *pu);
void pileup_args(unc_pileup *pu, PileupAccum *a);
bool pileup_hist_args(unc_pileup *pu, PileupHist *h);
}  // namespace unc

namespace {
// k_align_segments on every round of the DTW, while the round's paths are on the device (the next round reuses their buffer), and
// with an accumulator k_model_accum behind it, over the records the round has just written, and with a pile-up k_pileup_accum behind
// that, over the same records
struct SegmentsHook : DtwRoundHook {
    SegArgs args{};
    bool accumulate = false, pile = false, pile_hist = false;
    ModelAccum acc{};   // (with accumulate) everything but the round's jobs
    PileupAccum pu{};   // (with pile) the same
    PileupHist hist{};  // (with pile_hist) the pile-up's histogram, fed by k_pileup_hist_accum behind k_pileup_accum
    DevEvents ev;       // (timing only) two per round, one more with an accumulator, one more with a pile-up
    size_t per_round() const { return 2 + (accumulate ? 1 : 0) + (pile ? 1 : 0); }
    int round(const DtwJob *d_jobs, uint32_t n_jobs, uint64_t n_rows, const uint32_t *d_path, const unc_dtw_result_t *d_res, hipStream_t st) override {
        const size_t i = ev.e.size();
        HIPCHK(ev.create(i + per_round()));
        args.jobs = d_jobs; args.n_jobs = n_jobs; args.path = d_path; args.res = d_res;
        HIPCHK(ev.record(i, st));
        launch_align_segments(args, st);
        HIPCHK(hipGetLastError());
        HIPCHK(ev.record(i + 1, st));
        if (accumulate) {
            acc.jobs = d_jobs; acc.n_jobs = n_jobs;
            launch_model_accum(acc, n_rows, st);
            HIPCHK(hipGetLastError());
            HIPCHK(ev.record(i + 2, st));
        }
        if (pile) {
            pu.jobs = d_jobs; pu.n_jobs = n_jobs;
            launch_pileup_accum(pu, n_rows, st);
            HIPCHK(hipGetLastError());
            if (pile_hist) launch_pileup_hist_accum(pu, hist, n_rows, st);
            HIPCHK(hipGetLastError());
            HIPCHK(ev.record(i + per_round() - 1, st));
        }
        return UNC_OK;
    }
};

// One call of the pipeline: the call's record, and what the steps hand to each other.  The host vectors that an upload reads are kept
// here as well: they live as long as the call
struct AlignRun : AlignCall {
    AlignRows &rows;
    // check_and_lay_out: the options and parameters, resolved; the queries' records and the two totals
    unc_align_opts_t O;
    unc_dtw_params_t prm;
    unc_params_t P;
    // whole_events (with segments or the event tap): the kept events whole, and which became which column
    bool want_seg = false, want_tap = false, raw_mode = false, whole_events = false;
    DtwLayout layout{};                     // the DTW stage's: O.band with UNC_ALIGN_ADAPTIVE is the adaptive width, without it the half-width
    hipStream_t st = nullptr;
    std::vector<AlignQuery> hq;
    uint64_t n_gather = 0, n_cols = 0;
    // upload (d_events and d_col_evt: run_stages)
    const int16_t *d_raw = nullptr;
    const uint16_t *d_kmers = nullptr;
    const float *d_model = nullptr;
    DevBuf<int16_t> d_raw_own, d_gather;
    DevBuf<float> d_means, d_levels;
    DevBuf<AlignQuery> d_q;
    DevBuf<AlignRecord> d_rec;
    DevBuf<uint64_t> d_goff, d_moff, d_seg_off, d_smp_st;
    DevBuf<unc_calib_t> d_calib;
    DevBuf<unc_evt_info_t> d_info;
    DevBuf<unc_event_t> d_events;
    DevBuf<uint32_t> d_col_evt;
    std::vector<uint64_t> goff, moff, seg_off, smp_st;
    std::vector<unc_calib_t> qcal;
    DevReads rd{};
    DevEvents ev;                           // (timing only) around gather, event detection, mask + target + normalisation
    std::vector<AlignRecord> rec;           // read_back
    std::vector<DtwJob> jobs;               // plan_dtw
    std::vector<uint8_t> skip;
    std::vector<unc_dtw_result_t> dres;
    SegmentsHook hook;                      // set_up_segments
    DevBuf<unc_segment_t> d_seg;
    DevBuf<unc_seg_info_t> d_seginfo;
    DevBuf<unc_ref_stretch_t> d_stretches;  // (with a pile-up) the queries' coordinates

    AlignRun(const AlignCall &c, AlignRows &r) : AlignCall(c), rows(r) {}
    // the call's model on the host: the given one, or the template (both not complemented)
    const ModelTables &tables() const { return model ? model->fwd : dtw_model_default(); }

    // ---- arguments: everything is checked before the device is touched: this step makes no HIP call, and every later one may.
    // Then every query's checks in their order, and where its slice, its columns and its k-mers lie
    int check_and_lay_out() {
        if (!raw || !offsets || !calib || !queries || !results) return fail(UNC_ERR_ARG, "%s: null argument", who);
        if (path && !path_off) return fail(UNC_ERR_ARG, "%s: path without path_off", who);
        if (levels && !lev_off) return fail(UNC_ERR_ARG, "%s: levels without lev_off", who);
        if (segs && segs->seg && !segs->seg_off) return fail(UNC_ERR_ARG, "%s: seg without seg_off", who);
        if (segs && segs->events && !segs->evt_off) return fail(UNC_ERR_ARG, "%s: events without evt_off", who);
        want_seg = (segs && (segs->seg || segs->info)) || acc || pileup;
        want_tap = segs && segs->events;
        if (device < 0 || device >= DTW_MAX_DEVICES) return fail(UNC_ERR_ARG, "%s: device %d", who, device);
        if (acc && model_acc_device(acc) != device)
            return fail(UNC_ERR_ARG, "%s: the accumulator is on device %d, the call on device %d", who, model_acc_device(acc), device);
        memset(&O, 0, sizeof O);
        if (opts) O = *opts;
        if (O.flags & ~(UNC_ALIGN_DTW_PARAMS | UNC_ALIGN_NO_MASK | UNC_ALIGN_RAW | UNC_ALIGN_TARGET_MODEL | UNC_ALIGN_ADAPTIVE))
            return fail(UNC_ERR_ARG, "%s: unknown flags %#x", who, O.flags);
        prm = {UNC_DTW_NONE, UNC_DTW_R94D, 1.0f, 1.0f, 1.0f};        // dtw_test.cpp:76-78,162
        if (O.flags & UNC_ALIGN_DTW_PARAMS) prm = O.dtw;
        if (prm.subseq > UNC_DTW_COL) return fail(UNC_ERR_ARG, "%s: unknown subseq %u", who, prm.subseq);
        if (prm.cost > UNC_DTW_R94D) return fail(UNC_ERR_ARG, "%s: unknown cost %u", who, prm.cost);
        layout = (O.flags & UNC_ALIGN_ADAPTIVE) ? DtwLayout::adapt(O.band) : O.band ? DtwLayout::band(O.band) : DtwLayout::full();
        const uint32_t faults = dtw_mode_faults(layout, prm.subseq);
        if (faults & DTW_MODE_SUBSEQ) return fail(UNC_ERR_ARG, "%s: the band is global only (subseq %u)", who, prm.subseq);
        if (faults & DTW_MODE_WIDTH) return fail(UNC_ERR_ARG, "%s: an adaptive band of %u (64, 128 or 256)", who, O.band);
        if (params) P = *params;
        else unc_params_default(&P);
        if (P.window_length1 != UNC_WINDOW1 || P.window_length2 != UNC_WINDOW2)
            return fail(UNC_ERR_ARG, "%s: the event detector's windows must be %d and %d", who, UNC_WINDOW1, UNC_WINDOW2);
        raw_mode = (O.flags & UNC_ALIGN_RAW) != 0;
        whole_events = (want_seg || want_tap) && !raw_mode;
        st = (hipStream_t)stream;
        // (the timings are zeroed here: after the options' and parameters' checks, before a batch of no queries returns)
        memset(g_align_ms, 0, sizeof g_align_ms);
        g_seg_ms = 0;
        model_acc_set_timing(0);
        pileup_set_timing(0);
        if (n_queries == 0) return UNC_OK;
        for (uint32_t i = 0; i < n_reads; ++i)
            if (offsets[i + 1] < offsets[i]) return fail(UNC_ERR_ARG, "%s: offsets must ascend", who);
        hq.resize(n_queries);
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
            AlignQuery &a = hq[q];
            memset(&a, 0, sizeof a);
            if (int rc = rows.rows(q, &a.km_off, &a.n_km)) return rc;
            if (path && path_off[q + 1] < path_off[q]) return fail(UNC_ERR_ARG, "%s: path_off must ascend", who);
            if (levels && lev_off[q + 1] < lev_off[q]) return fail(UNC_ERR_ARG, "%s: lev_off must ascend", who);
            if (segs && segs->seg && segs->seg_off[q + 1] < segs->seg_off[q]) return fail(UNC_ERR_ARG, "%s: seg_off must ascend", who);
            if (want_tap && segs->evt_off[q + 1] < segs->evt_off[q]) return fail(UNC_ERR_ARG, "%s: evt_off must ascend", who);
            a.src_off = offsets[u.read] - offsets[0] + u.smp_st;
            a.n_smp = (uint32_t)(en - u.smp_st);
            a.dst_off = n_gather;
            a.col_off = n_cols;
            // (peak_detect emits a peak once it lies more than window_length / 2 samples back and then starts afresh: the short detector
            // fires at most every third sample, the long one every fifth.  An event that finds its room full is reported by read_back)
            a.col_cap = raw_mode ? a.n_smp : a.n_smp / 2 + 16;
            a.calib = calib[u.read];
            n_gather += a.n_smp;
            n_cols += a.col_cap;
        }
        return rows.check();
    }

    // ---- device: every allocation and upload that the stages need is queued here, before the first timing event is recorded, so that
    // the spans between the events hold kernels only
    int upload() {
        HIPCHK(hipSetDevice(device));
        if (int rc = model ? model_device(model, device, &d_model) : dtw_model_device(device, &d_model)) return rc;
        d_raw = raw + offsets[0];
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
            rd.tgt_mean = tables().mean; rd.tgt_stdv = tables().stdv;       // (k_events' own scale and shift are not used here)
        }
        HIPCHK(ev.create(4));
        return UNC_OK;
    }

    // a. the slices, then event detection on each;  b. - d. mask, target, normalisation
    int run_stages() {
        HIPCHK(ev.record(0, st));
        launch_align_gather(d_raw, d_q.p, n_queries, raw_mode ? nullptr : d_gather.p, raw_mode ? d_means.p : nullptr, st);
        HIPCHK(hipGetLastError());
        HIPCHK(ev.record(1, st));
        if (!raw_mode) {
            // as few slices per wavefront as a grid of 2048 wavefronts allows (the kernel is sequential per slice)
            const uint32_t rpw = std::min<uint32_t>(64u, std::max<uint32_t>(1u, (n_queries + 2047u) / 2048u));
            if (whole_events) {
                HIPCHK(d_events.alloc(n_cols)); HIPCHK(d_col_evt.alloc(n_cols));
                launch_events_full(rd, P, d_events.p, st, rpw);
            } else launch_events(rd, P, st, rpw);
            HIPCHK(hipGetLastError());
        }
        HIPCHK(ev.record(2, st));
        AlignPrep ap{};
        ap.queries = d_q.p; ap.n_queries = n_queries; ap.flags = O.flags;
        ap.info = raw_mode ? nullptr : d_info.p;
        ap.means = d_means.p;
        ap.levels = d_levels.p;
        ap.kmers = d_kmers; ap.model = d_model;
        ap.model_mean = tables().mean; ap.model_stdv = tables().stdv;
        ap.rec = d_rec.p;
        ap.col_evt = whole_events ? d_col_evt.p : nullptr;
        launch_align_prep(ap, st);
        HIPCHK(hipGetLastError());
        HIPCHK(ev.record(3, st));
        return UNC_OK;
    }

    // one 32-byte record per query (the planner lays out back-pointers by column counts), the stages' times, and the overflow report
    int read_back() {
        std::vector<unc_evt_info_t> info;
        HIPCHK(download(rec, d_rec.p, n_queries, st));
        if (!raw_mode) HIPCHK(download(info, d_info.p, n_queries, st));
        HIPCHK(hipStreamSynchronize(st));
        for (int i = 0; i < 3; ++i) HIPCHK(ev.elapsed(i, i + 1, &g_align_ms[i]));
        for (uint32_t q = 0; q < n_queries && !raw_mode; ++q)
            if (info[q].pad) return fail(UNC_ERR_OVERFLOW, "%s: query %u has more events than its room of %u", who, q, hq[q].col_cap);
        return UNC_OK;
    }

    // e. the DTW over the levels where they lie: a job per query, `skip` for those that get none.  The first step that writes results
    void plan_dtw() {
        jobs.resize(n_queries);
        skip.assign(n_queries, 0);
        dres.assign(n_queries, unc_dtw_result_t{});
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
    }

    // f. (with segments) what k_align_segments needs on every round's paths.  The records' layout on the device, from 0: a query's room
    // there is the caller's, or its k-mers if those are fewer (a path has no more rows); without seg no room at all, and info alone is
    // filled.  With an accumulator or a pile-up the room is the query's k-mers whatever the caller's: every record is made, for
    // k_model_accum and k_pileup_accum
    int set_up_segments() {
        const bool caller_seg = segs && segs->seg;
        seg_off.assign((size_t)n_queries + 1, 0);
        smp_st.resize(n_queries);
        for (uint32_t q = 0; q < n_queries; ++q) {
            smp_st[q] = queries[q].smp_st;
            const uint64_t room = caller_seg ? std::min<uint64_t>(segs->seg_off[q + 1] - segs->seg_off[q], hq[q].n_km) : 0;
            seg_off[q + 1] = seg_off[q] + (acc || pileup ? hq[q].n_km : room);
        }
        HIPCHK(d_seg.alloc(seg_off[n_queries])); HIPCHK(d_seginfo.alloc(n_queries));
        HIPCHK(d_seg_off.alloc(seg_off.size())); HIPCHK(d_smp_st.alloc(n_queries));
        HIPCHK(hipMemcpyAsync(d_seg_off.p, seg_off.data(), seg_off.size() * 8, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(d_smp_st.p, smp_st.data(), smp_st.size() * 8, hipMemcpyHostToDevice, st));
        SegArgs &sa = hook.args;
        sa.raw = raw_mode ? 1u : 0u;
        sa.queries = d_q.p; sa.rec = d_rec.p;
        sa.events = d_events.p; sa.means = d_means.p; sa.col_evt = d_col_evt.p;
        sa.smp_st = d_smp_st.p; sa.seg_off = d_seg_off.p; sa.seg = d_seg.p; sa.info = d_seginfo.p;
        if (acc) {
            hook.accumulate = true;
            model_acc_args(acc, &hook.acc);
            hook.acc.kmers = d_kmers; hook.acc.info = d_seginfo.p; hook.acc.queries = d_q.p; hook.acc.seg_off = d_seg_off.p; hook.acc.seg = d_seg.p;
        }
        if (pileup) {
            HIPCHK(d_stretches.alloc(n_queries));
            HIPCHK(hipMemcpyAsync(d_stretches.p, stretches, (size_t)n_queries * sizeof(unc_ref_stretch_t), hipMemcpyHostToDevice, st));
            hook.pile = true;
            pileup_args(pileup, &hook.pu);
            hook.pile_hist = pileup_hist_args(pileup, &hook.hist);
            hook.pu.info = d_seginfo.p; hook.pu.queries = d_q.p; hook.pu.seg_off = d_seg_off.p; hook.pu.seg = d_seg.p;
            hook.pu.stretches = d_stretches.p;
        }
        return UNC_OK;
    }

    // the DTW's rounds (with segments: k_align_segments on each), their times, and the results of the queries that were in one
    int run_dtw() {
        DtwCall c{};
        c.device = device; c.st = st; c.n = n_queries; c.d_events = d_levels.p; c.d_kmers = d_kmers; c.jobs = jobs.data(); c.skip = skip.data();
        c.prm = &prm; c.layout = layout; c.workspace_bytes = workspace_bytes; c.res = dres.data(); c.path = path; c.path_off = path_off;
        c.hook = want_seg ? &hook : nullptr; c.model = model;
        if (int rc = dtw_run_device(c)) return rc;
        (void)unc_dtw_last_timing(&g_align_ms[3], nullptr, nullptr);
        const size_t per_round = hook.per_round();
        float acc_ms = 0, pile_ms = 0;
        for (size_t i = 0; i + per_round <= hook.ev.e.size(); i += per_round) {       // (g_seg_ms is 0 since check_and_lay_out)
            float t = 0;
            HIPCHK(hook.ev.elapsed(i, i + 1, &t));
            g_seg_ms += t;
            if (hook.accumulate) {
                HIPCHK(hook.ev.elapsed(i + 1, i + 2, &t));
                acc_ms += t;
            }
            if (hook.pile) {
                HIPCHK(hook.ev.elapsed(i + per_round - 2, i + per_round - 1, &t));
                pile_ms += t;
            }
        }
        model_acc_set_timing(acc_ms);
        pileup_set_timing(pile_ms);
        for (uint32_t q = 0; q < n_queries; ++q) {
            if (skip[q]) continue;
            results[q].dtw = dres[q];
            results[q].status = dres[q].status;
        }
        return UNC_OK;
    }

    // ---- the outputs on request: one copy of a whole device array each, dealt out per query on the host (deal_out, unc_host_util.h),
    // so that nothing outside a query's count is written
    int hand_over() {
        const bool caller_seg = segs && segs->seg;
        if (segs && (segs->seg || segs->info)) {     // the rows' counts first, then the records by them
            std::vector<unc_seg_info_t> info;
            HIPCHK(download(info, d_seginfo.p, n_queries, st));
            HIPCHK(hipStreamSynchronize(st));
            for (uint32_t q = 0; q < n_queries; ++q) {
                const uint32_t s = results[q].status;
                unc_seg_info_t &inf = info[q];
                // (a query that was in no round, or whose path has no start, has no rows: its record on the device may never have been written)
                if (skip[q] || (s != UNC_DTW_OK && s != UNC_DTW_PATH_TRUNCATED && s != UNC_DTW_REF_END)) { inf.row_first = 0; inf.n_rows = 0; inf.status = UNC_SEG_NONE; inf.pad = 0; }
                if (!caller_seg && inf.status == UNC_SEG_TRUNCATED) inf.status = UNC_SEG_OK;       // (no records were asked for: none is missing)
                // (with an accumulator or a pile-up the room on the device is not the caller's: the status goes by the caller's)
                if (caller_seg && inf.status == UNC_SEG_OK && inf.n_rows > segs->seg_off[q + 1] - segs->seg_off[q]) inf.status = UNC_SEG_TRUNCATED;
                if (segs->info) segs->info[q] = inf;
            }
            if (caller_seg)
                HIPCHK(deal_out(d_seg.p, (size_t)seg_off[n_queries], st, n_queries,
                                [&](uint32_t q) { return std::min<uint64_t>(info[q].n_rows, std::min<uint64_t>(seg_off[q + 1] - seg_off[q],
                                                                                                            segs->seg_off[q + 1] - segs->seg_off[q])); },
                                [&](uint32_t q) { return seg_off[q]; }, [&](uint32_t q) { return segs->seg + segs->seg_off[q]; }));
        }
        if (want_tap) {     // the tap: the columns as events.  It transforms what it copies, so the loop is its own
            std::vector<unc_event_t> hev;
            std::vector<uint32_t> hce;
            std::vector<float> hsm;
            if (raw_mode) HIPCHK(download(hsm, d_means.p, (size_t)n_cols, st));
            else {
                HIPCHK(download(hev, d_events.p, (size_t)n_cols, st));
                HIPCHK(download(hce, d_col_evt.p, (size_t)n_cols, st));
            }
            HIPCHK(hipStreamSynchronize(st));
            for (uint32_t q = 0; q < n_queries; ++q) {
                const uint64_t got = std::min<uint64_t>(results[q].n_kept, segs->evt_off[q + 1] - segs->evt_off[q]);
                unc_event_t *out = segs->events + segs->evt_off[q];
                for (uint64_t c = 0; c < got; ++c) {
                    if (raw_mode) out[c] = unc_event_t{hsm[hq[q].col_off + c], 0.0f, (uint32_t)c, 1u};
                    else out[c] = hev[hq[q].col_off + hce[hq[q].col_off + c]];
                }
            }
        }
        if (levels)         // the tap: the columns the DTW read
            HIPCHK(deal_out(d_levels.p, (size_t)n_cols, st, n_queries,
                            [&](uint32_t q) { return std::min<uint64_t>(results[q].n_kept, lev_off[q + 1] - lev_off[q]); },
                            [&](uint32_t q) { return hq[q].col_off; }, [&](uint32_t q) { return levels + lev_off[q]; }));
        return UNC_OK;
    }
};
}  // namespace

// The pipeline, from the arguments' checks to the results.  The queries' rows are `rows`' business (align_dev.h).
int unc::align_run(const AlignCall &c, AlignRows &rows) {
    AlignRun s(c, rows);
    if (int rc = s.check_and_lay_out()) return rc;
    if (c.n_queries == 0) return UNC_OK;
    if (int rc = s.upload()) return rc;
    if (int rc = s.run_stages()) return rc;
    if (int rc = s.read_back()) return rc;
    s.plan_dtw();
    if (int rc = s.want_seg ? s.set_up_segments() : UNC_OK) return rc;
    if (int rc = s.run_dtw()) return rc;
    return s.hand_over();
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

// The one way in: a call's record (unc_align_call_t, include/uncalled_hip.h) under the name of the entry point that filled it
static int align_dispatch(const unc_align_call_t &u, const char *who, unc_pileup_t *pileup = nullptr);

extern "C" int unc_align_call(const unc_align_call_t *call) {
    static const char *who = "unc_align_call";
    if (!call) return fail(UNC_ERR_ARG, "%s: null argument", who);
    if (call->size < sizeof(uint32_t) || call->size > sizeof(unc_align_call_t))
        return fail(UNC_ERR_ARG, "%s: size %u is not that of a record of this library (%zu)", who, call->size, sizeof(unc_align_call_t));
    unc_align_call_t u;
    memset(&u, 0, sizeof u);
    memcpy(&u, call, call->size);
    if ((u.kmers != nullptr) == (u.refseq != nullptr)) return fail(UNC_ERR_ARG, "%s: rows come as kmers or as refseq, one of the two", who);
    return align_dispatch(u, who);
}

// the parameters that all four entry points below share, as a record
static unc_align_call_t align_record(int device, const unc_params_t *params, const unc_align_opts_t *opts, uint32_t n_reads, const int16_t *raw,
                                     const uint64_t *offsets, const unc_calib_t *calib, int on_device, uint32_t n_queries,
                                     const unc_align_query_t *queries, uint64_t workspace_bytes, unc_align_result_t *results, float *levels,
                                     const uint64_t *lev_off, uint32_t *path, const uint64_t *path_off, const unc_align_segments_t *segs, void *stream) {
    unc_align_call_t u;
    memset(&u, 0, sizeof u);
    u.size = sizeof u; u.device = device; u.params = params; u.opts = opts; u.n_reads = n_reads; u.on_device = on_device; u.raw = raw;
    u.offsets = offsets; u.calib = calib; u.n_queries = n_queries; u.queries = queries; u.workspace_bytes = workspace_bytes;
    u.results = results; u.levels = levels; u.lev_off = lev_off; u.path = path; u.path_off = path_off; u.segs = segs; u.stream = stream;
    return u;
}

extern "C" int unc_align_batch(int device, const unc_params_t *params, const unc_align_opts_t *opts, uint32_t n_reads, const int16_t *raw,
                               const uint64_t *offsets, const unc_calib_t *calib, int on_device, uint32_t n_queries,
                               const unc_align_query_t *queries, const uint16_t *kmers, const uint64_t *km_off, uint64_t workspace_bytes,
                               unc_align_result_t *results, float *levels, const uint64_t *lev_off, uint32_t *path, const uint64_t *path_off,
                               void *stream) {
    unc_align_call_t u = align_record(device, params, opts, n_reads, raw, offsets, calib, on_device, n_queries, queries, workspace_bytes, results,
                                      levels, lev_off, path, path_off, nullptr, stream);
    u.kmers = kmers; u.km_off = km_off;
    return align_dispatch(u, "unc_align_batch");
}

extern "C" int unc_align_segments_batch(int device, const unc_params_t *params, const unc_align_opts_t *opts, uint32_t n_reads, const int16_t *raw,
                                        const uint64_t *offsets, const unc_calib_t *calib, int on_device, uint32_t n_queries,
                                        const unc_align_query_t *queries, const uint16_t *kmers, const uint64_t *km_off, uint64_t workspace_bytes,
                                        unc_align_result_t *results, float *levels, const uint64_t *lev_off, uint32_t *path,
                                        const uint64_t *path_off, const unc_align_segments_t *out, void *stream) {
    if (!out) return fail(UNC_ERR_ARG, "%s: null argument", "unc_align_segments_batch");
    unc_align_call_t u = align_record(device, params, opts, n_reads, raw, offsets, calib, on_device, n_queries, queries, workspace_bytes, results,
                                      levels, lev_off, path, path_off, out, stream);
    u.kmers = kmers; u.km_off = km_off;
    return align_dispatch(u, "unc_align_segments_batch");
}

// unc_align_ref_batch and the packed reference: unc_refseq.cpp and k_refseq.hip are compiled as part of this translation unit, so that
// every build of the alignment sources holds them
#include "unc_refseq.cpp"

// rows as coordinates (u.refseq; the route of unc_refseq.cpp), or the caller's k-mers, uploaded
static int align_dispatch(const unc_align_call_t &u, const char *who, unc_pileup_t *pileup) {
    const AlignCall c{who, u.device, u.params, u.opts, u.n_reads, u.raw, u.offsets, u.calib, u.on_device, u.n_queries, u.queries,
                      u.workspace_bytes, u.results, u.levels, u.lev_off, u.path, u.path_off, u.stream, u.segs, u.model, u.accumulate,
                      pileup, pileup ? u.stretches : nullptr};
    if (u.refseq || u.stretches) return align_ref(c, u.refseq, u.stretches, u.kmers_out, u.kmers_off);
    if (!u.raw || !u.offsets || !u.calib || !u.queries || !u.kmers || !u.km_off || !u.results) return fail(UNC_ERR_ARG, "%s: null argument", who);
    UploadedRows rows(u.kmers, u.km_off, u.n_queries);
    return align_run(c, rows);
}

// the training accumulator's host side is compiled as part of this translation unit in the same way
#include "unc_model_acc.cpp"
// and so is the pile-up's
#include "unc_pileup.cpp"
// with its histograms and their Kolmogorov-Smirnov distance
#include "unc_pileup_hist.cpp"

// unc_align_call with a pile-up behind the segments (and behind the accumulator, when there is one): the same record, the same body
extern "C" int unc_align_pileup_call(const unc_align_call_t *call, unc_pileup_t *pileup) {
    static const char *who = "unc_align_pileup_call";
    if (!pileup) return unc_align_call(call);
    if (!call) return fail(UNC_ERR_ARG, "%s: null argument", who);
    if (call->size < sizeof(uint32_t) || call->size > sizeof(unc_align_call_t))
        return fail(UNC_ERR_ARG, "%s: size %u is not that of a record of this library (%zu)", who, call->size, sizeof(unc_align_call_t));
    unc_align_call_t u;
    memset(&u, 0, sizeof u);
    memcpy(&u, call, call->size);
    if (u.kmers || !u.refseq || !u.stretches)
        return fail(UNC_ERR_ARG, "%s: a pile-up needs the rows as refseq and stretches: k-mer arrays have no coordinates", who);
    if (pileup_refseq(pileup) != u.refseq || pileup_device(pileup) != u.refseq->device)
        return fail(UNC_ERR_ARG, "%s: the pile-up was made for another packed reference or device", who);
    return align_dispatch(u, who, pileup);
}
