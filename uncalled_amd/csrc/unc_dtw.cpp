// Host side of the DTW entry points of include/uncalled_hip.h: argument checks, the queue of alignments in descending chain (cells,
// or the steps of a band), the split of a batch into rounds that fit the workspace, and BwaIndex::get_kmers on the packed reference
// (host only).
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <mutex>
#include <numeric>
#include <string>
#include <vector>

#include "dtw_dev.h"
#include "unc_host_util.h"
#include "unc_model.h"

using namespace unc;

// ------------------------------------------------------------------ the template model
// PoreModel(vector, cmpl=false) of the compiled-in pairs, through the one builder (unc_model.h): rows not complemented -- row k here
// is row k ^ 0x3FF of the index's tables (unc_host.cpp).
const ModelTables &unc::dtw_model_default() {
    static ModelTables tab;
    static std::once_flag once;
    std::call_once(once, [] {
        float pairs[2 * UNC_NKMER];
        model_default_pairs(pairs);
        model_build_tables(pairs, false, &tab);
    });
    return tab;
}
const float *unc::dtw_model_host() { return dtw_model_default().tab; }

extern "C" void unc_dtw_model_tables(float *means1024, float *vars_x2_1024, float *lognorm1024) {
    const float *t = dtw_model_host();
    if (means1024) memcpy(means1024, t, UNC_NKMER * 4);
    if (vars_x2_1024) memcpy(vars_x2_1024, t + UNC_NKMER, UNC_NKMER * 4);
    if (lognorm1024) memcpy(lognorm1024, t + 2 * UNC_NKMER, UNC_NKMER * 4);
}

// one copy per device, uploaded by the first batch there and kept for the life of the process
static std::mutex g_model_mutex;
static DevBuf<float> *g_model[DTW_MAX_DEVICES];
int unc::dtw_model_device(int device, const float **out) {
    std::lock_guard<std::mutex> lk(g_model_mutex);
    if (!g_model[device]) {
        DevBuf<float> buf;
        HIPCHK(buf.alloc(3 * UNC_NKMER));
        HIPCHK(hipMemcpy(buf.p, dtw_model_host(), 3 * UNC_NKMER * sizeof(float), hipMemcpyHostToDevice));
        g_model[device] = new DevBuf<float>(std::move(buf));
    }
    *out = g_model[device]->p;
    return UNC_OK;
}

// ------------------------------------------------------------------ batch
static thread_local float g_last_ms = 0;
static thread_local uint32_t g_last_rounds = 0;
static thread_local uint64_t g_last_crumb_bytes = 0;

extern "C" int unc_dtw_last_timing(float *ms_kernel, uint32_t *rounds, uint64_t *crumb_bytes) {
    if (ms_kernel) *ms_kernel = g_last_ms;
    if (rounds) *rounds = g_last_rounds;
    if (crumb_bytes) *crumb_bytes = g_last_crumb_bytes;
    return UNC_OK;
}

namespace {
// One call of dtw_run_device (dtw_dev.h): the call's record, and what the steps hand to each other
struct DtwRun : DtwCall {
    // plan_queue: the workspace resolved, every alignment's words, the queue and how far the rounds have taken it
    uint64_t workspace = 0;
    std::vector<uint64_t> words;
    std::vector<uint32_t> todo;
    size_t at = 0;
    // set_up_device (d_crumbs, d_lines, d_jobs and d_path grow with the rounds)
    const float *d_model = nullptr;
    int n_cu = 1;
    DevBuf<float> d_lines; DevBuf<uint32_t> d_crumbs, d_path, d_next; DevBuf<DtwJob> d_jobs; DevBuf<unc_dtw_result_t> d_res;
    DevEvents ev;                           // (timing only) around a round's kernel
    // next_round: the round's jobs with their offsets, and its totals in words, floats, pairs and rows
    std::vector<DtwJob> round;
    std::vector<uint32_t> caller_cap;       // (with a hook: what the caller's room holds of each of the round's paths)
    uint64_t w = 0, lines = 0, pairs = 0, rows = 0;
    // read_back_round
    std::vector<uint32_t> h_path;
    std::vector<unc_dtw_result_t> h_res;

    explicit DtwRun(const DtwCall &c) : DtwCall(c) {}

    // the queue: descending chain, so that the longest alignments start first and none sits alone at the tail.  What is left out
    // gets its status here
    int plan_queue() {
        std::vector<uint64_t> chain(n);
        words.resize(n);
        for (uint32_t a = 0; a < n; ++a) {
            chain[a] = layout.chain(jobs[a].rows, jobs[a].cols);
            words[a] = layout.words(jobs[a].rows, jobs[a].cols);
        }
        workspace = workspace_bytes;
        if (workspace == 0) {
            size_t free_b = 0, total_b = 0;
            HIPCHK(hipMemGetInfo(&free_b, &total_b));
            workspace = free_b / 2;
        }
        std::vector<uint32_t> order(n);
        std::iota(order.begin(), order.end(), 0u);
        std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return chain[x] > chain[y]; });
        for (uint32_t a : order) {
            if (skip && skip[a]) continue;
            const bool narrow = !layout.feasible(jobs[a].rows, jobs[a].cols);
            if (narrow || words[a] * 4 > workspace) {
                res[a].score = 0; res[a].mean_score = 0; res[a].path_len = 0; res[a].pad = 0;
                res[a].status = narrow ? UNC_DTW_BAND_TOO_NARROW : UNC_DTW_TOO_LARGE;
            } else todo.push_back(a);
        }
        return UNC_OK;
    }

    // what every round uses: the model's tables, the results, the queue's counter, the events and the CU count
    int set_up_device() {
        if (int rc = model ? model_device(model, device, &d_model) : dtw_model_device(device, &d_model)) return rc;
        HIPCHK(d_res.alloc(n)); HIPCHK(d_next.alloc(1));
        hipDeviceProp_t prop;
        HIPCHK(hipGetDeviceProperties(&prop, device));
        n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 1;
        HIPCHK(ev.create(2));
        return UNC_OK;
    }

    // a round: the next alignments of the queue whose back-pointers fit the workspace together (one at least)
    void next_round() {
        round.clear(); caller_cap.clear();
        w = 0; lines = 0; pairs = 0; rows = 0;
        while (at < todo.size() && (round.empty() || (w + words[todo[at]]) * 4 <= workspace)) {
            DtwJob j = jobs[todo[at]];
            j.crumb_off = w; j.line_off = lines; j.path_off = pairs;
            caller_cap.push_back(j.path_cap);
            if (hook) j.path_cap = j.rows + j.cols - 1;          // (both below 2^31)
            w += words[todo[at]];
            lines += layout.line_floats(j.cols);
            pairs += j.path_cap;
            rows += j.rows;
            round.push_back(j);
            ++at;
        }
    }

    // the round's buffers, its jobs on the device, the kernel between the two events, and the hook
    int launch_round() {
        const uint32_t nr = (uint32_t)round.size();
        HIPCHK(d_crumbs.reserve(w)); HIPCHK(d_lines.reserve(lines)); HIPCHK(d_jobs.reserve(nr));
        const bool dev_path = path || hook;
        if (dev_path) HIPCHK(d_path.reserve(std::max<uint64_t>(2 * pairs, 2)));
        HIPCHK(hipMemcpyAsync(d_jobs.p, round.data(), nr * sizeof(DtwJob), hipMemcpyHostToDevice, st));
        HIPCHK(hipMemsetAsync(d_next.p, 0, sizeof(uint32_t), st));
        DtwBatch b{};
        b.events = d_events; b.kmers = d_kmers; b.model = d_model; b.jobs = d_jobs.p; b.n_jobs = nr;
        b.subseq = prm->subseq; b.layout = layout; b.dw = prm->dw; b.hw = prm->hw; b.vw = prm->vw;
        b.crumbs = d_crumbs.p; b.lines = d_lines.p; b.path = dev_path ? d_path.p : nullptr; b.res = d_res.p; b.next = d_next.p;
        const uint32_t grid = std::min<uint32_t>(nr, (uint32_t)n_cu * 16u);
        HIPCHK(ev.record(0, st));
        launch_dtw(b, prm->cost, grid, st);
        HIPCHK(hipGetLastError());
        HIPCHK(ev.record(1, st));
        return hook ? hook->round(d_jobs.p, nr, rows, d_path.p, d_res.p, st) : UNC_OK;
    }

    // the round's results and paths on the host, its time, and what the caller gets of each
    int read_back_round() {
        h_path.resize(path ? 2 * pairs : 0);
        // (the results of this round's alignments lie scattered over d_res: the whole array is small)
        HIPCHK(download(h_res, d_res.p, n, st));
        if (path && pairs) HIPCHK(hipMemcpyAsync(h_path.data(), d_path.p, 2 * pairs * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        float ms = 0;
        HIPCHK(ev.elapsed(0, 1, &ms));
        g_last_ms += ms;
        g_last_rounds += 1;
        g_last_crumb_bytes = std::max<uint64_t>(g_last_crumb_bytes, w * 4);
        for (size_t k = 0; k < round.size(); ++k) {
            const DtwJob &j = round[k];
            unc_dtw_result_t r = h_res[j.out];
            r.mean_score = r.score / (float)r.path_len;          // dtw.hpp:130-132
            // (with a hook the kernel had room for every pair, or was asked for a path the caller did not want: the status it gives
            // without one, k_dtw.hip -- UNC_DTW_LEFT_BAND first, then the caller's room)
            if (hook && (r.status == UNC_DTW_OK || r.status == UNC_DTW_REF_END) && path && r.path_len > caller_cap[k]) r.status = UNC_DTW_PATH_TRUNCATED;
            res[j.out] = r;
            if (path) {
                const uint64_t got = std::min<uint64_t>(r.path_len, caller_cap[k]);
                memcpy(path + 2 * path_off[j.out], h_path.data() + 2 * j.path_off, got * 2 * sizeof(uint32_t));
            }
        }
        return UNC_OK;
    }
};
}  // namespace

int unc::dtw_run_device(const DtwCall &c) {
    g_last_ms = 0; g_last_rounds = 0; g_last_crumb_bytes = 0;
    DtwRun s(c);
    if (int rc = s.plan_queue()) return rc;
    if (s.todo.empty()) return UNC_OK;
    if (int rc = s.set_up_device()) return rc;
    while (s.at < s.todo.size()) {
        s.next_round();
        if (int rc = s.launch_round()) return rc;
        if (int rc = s.read_back_round()) return rc;
    }
    return UNC_OK;
}

// the body of the four entry points below: the rules of a layout (dtw_mode_faults) are reported by its entry point, in its words
static int dtw_batch(int device, const unc_model *model, uint32_t n, const float *events, const uint64_t *ev_off, const uint16_t *kmers, const uint64_t *km_off,
                     const unc_dtw_params_t *prm, DtwLayout layout, uint64_t workspace_bytes, unc_dtw_result_t *res, uint32_t *path,
                     const uint64_t *path_off, void *stream) {
    // ---- arguments: everything is checked before the device is touched
    if (!events || !ev_off || !kmers || !km_off || !prm || !res) return fail(UNC_ERR_ARG, "unc_dtw_batch: null argument");
    if (path && !path_off) return fail(UNC_ERR_ARG, "unc_dtw_batch: path without path_off");
    if (device < 0 || device >= DTW_MAX_DEVICES) return fail(UNC_ERR_ARG, "unc_dtw_batch: device %d", device);
    if (prm->subseq > UNC_DTW_COL) return fail(UNC_ERR_ARG, "unc_dtw_batch: unknown subseq %u", prm->subseq);
    if (prm->cost > UNC_DTW_R94D) return fail(UNC_ERR_ARG, "unc_dtw_batch: unknown cost %u", prm->cost);
    g_last_ms = 0; g_last_rounds = 0; g_last_crumb_bytes = 0;
    if (n == 0) return UNC_OK;
    std::vector<DtwJob> jobs(n);
    for (uint32_t a = 0; a < n; ++a) {
        if (ev_off[a + 1] <= ev_off[a]) return fail(UNC_ERR_ARG, "unc_dtw_batch: alignment %u has no events", a);
        if (km_off[a + 1] <= km_off[a]) return fail(UNC_ERR_ARG, "unc_dtw_batch: alignment %u has no k-mers", a);
        if (a && (ev_off[a] < ev_off[a - 1] || km_off[a] < km_off[a - 1])) return fail(UNC_ERR_ARG, "unc_dtw_batch: offsets must ascend");
        const uint64_t cols = ev_off[a + 1] - ev_off[a], rows = km_off[a + 1] - km_off[a];
        if (cols >= (1ull << 31) || rows >= (1ull << 31)) return fail(UNC_ERR_ARG, "unc_dtw_batch: alignment %u: 2^31 or more rows or columns", a);
        if (path && path_off[a + 1] < path_off[a]) return fail(UNC_ERR_ARG, "unc_dtw_batch: path_off must ascend");
        DtwJob &j = jobs[a];
        j.ev_off = ev_off[a] - ev_off[0];
        j.km_off = km_off[a] - km_off[0];
        j.rows = (uint32_t)rows; j.cols = (uint32_t)cols;
        j.out = a;
        const uint64_t room = path ? path_off[a + 1] - path_off[a] : 0;
        j.path_cap = (uint32_t)std::min<uint64_t>(room, rows + cols - 1);
    }
    const uint64_t n_ev = ev_off[n] - ev_off[0], n_km = km_off[n] - km_off[0];
    for (uint64_t i = 0; i < n_km; ++i)
        if (kmers[km_off[0] + i] >= UNC_NKMER) return fail(UNC_ERR_ARG, "unc_dtw_batch: k-mer %u at %llu is not below %d", kmers[km_off[0] + i],
                                                           (unsigned long long)(km_off[0] + i), UNC_NKMER);

    // ---- device
    HIPCHK(hipSetDevice(device));
    hipStream_t st = (hipStream_t)stream;
    DevBuf<float> d_events;
    DevBuf<uint16_t> d_kmers;
    HIPCHK(d_events.alloc(n_ev)); HIPCHK(d_kmers.alloc(n_km));
    HIPCHK(hipMemcpyAsync(d_events.p, events + ev_off[0], n_ev * sizeof(float), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_kmers.p, kmers + km_off[0], n_km * sizeof(uint16_t), hipMemcpyHostToDevice, st));
    DtwCall c{};
    c.device = device; c.st = st; c.n = n; c.d_events = d_events.p; c.d_kmers = d_kmers.p; c.jobs = jobs.data();
    c.prm = prm; c.layout = layout; c.workspace_bytes = workspace_bytes; c.res = res; c.path = path; c.path_off = path_off; c.model = model;
    return dtw_run_device(c);
}

extern "C" int unc_dtw_batch(int device, uint32_t n, const float *events, const uint64_t *ev_off, const uint16_t *kmers,
                             const uint64_t *km_off, const unc_dtw_params_t *prm, uint64_t workspace_bytes, unc_dtw_result_t *res,
                             uint32_t *path, const uint64_t *path_off, void *stream) {
    return dtw_batch(device, nullptr, n, events, ev_off, kmers, km_off, prm, DtwLayout::full(), workspace_bytes, res, path, path_off, stream);
}

extern "C" int unc_dtw_band_batch(int device, uint32_t n, const float *events, const uint64_t *ev_off, const uint16_t *kmers,
                                  const uint64_t *km_off, const unc_dtw_params_t *prm, uint32_t band, uint64_t workspace_bytes,
                                  unc_dtw_result_t *res, uint32_t *path, const uint64_t *path_off, void *stream) {
    const DtwLayout layout = DtwLayout::band(band);
    const uint32_t faults = dtw_mode_faults(layout, prm ? prm->subseq : UNC_DTW_NONE);
    if (faults & DTW_MODE_WIDTH) return fail(UNC_ERR_ARG, "unc_dtw_band_batch: a band of 0 (unc_dtw_batch is the full matrix)");
    if (faults & DTW_MODE_SUBSEQ) return fail(UNC_ERR_ARG, "unc_dtw_band_batch: the band is global only (subseq %u)", prm->subseq);
    return dtw_batch(device, nullptr, n, events, ev_off, kmers, km_off, prm, layout, workspace_bytes, res, path, path_off, stream);
}

extern "C" int unc_dtw_adapt_batch(int device, uint32_t n, const float *events, const uint64_t *ev_off, const uint16_t *kmers,
                                   const uint64_t *km_off, const unc_dtw_params_t *prm, uint32_t band, uint64_t workspace_bytes,
                                   unc_dtw_result_t *res, uint32_t *path, const uint64_t *path_off, void *stream) {
    const DtwLayout layout = DtwLayout::adapt(band);
    const uint32_t faults = dtw_mode_faults(layout, prm ? prm->subseq : UNC_DTW_NONE);
    if (faults & DTW_MODE_WIDTH) return fail(UNC_ERR_ARG, "unc_dtw_adapt_batch: a band of %u (64, 128 or 256)", band);
    if (faults & DTW_MODE_SUBSEQ)
        return fail(UNC_ERR_ARG, "unc_dtw_adapt_batch: the adaptive band has a global start and an open end of its own (subseq %u)", prm->subseq);
    return dtw_batch(device, nullptr, n, events, ev_off, kmers, km_off, prm, layout, workspace_bytes, res, path, path_off, stream);
}

// either of the first two above, by `band`, with the costs of a model (null: the template's)
extern "C" int unc_dtw_model_batch(int device, const unc_model_t *model, uint32_t n, const float *events, const uint64_t *ev_off,
                                   const uint16_t *kmers, const uint64_t *km_off, const unc_dtw_params_t *prm, uint32_t band,
                                   uint64_t workspace_bytes, unc_dtw_result_t *res, uint32_t *path, const uint64_t *path_off, void *stream) {
    const DtwLayout layout = band ? DtwLayout::band(band) : DtwLayout::full();
    if (dtw_mode_faults(layout, prm ? prm->subseq : UNC_DTW_NONE) & DTW_MODE_SUBSEQ)
        return fail(UNC_ERR_ARG, "unc_dtw_model_batch: the band is global only (subseq %u)", prm->subseq);
    return dtw_batch(device, model, n, events, ev_off, kmers, km_off, prm, layout, workspace_bytes, res, path, path_off, stream);
}

// ------------------------------------------------------------------ BwaIndex::get_kmers
extern "C" int unc_ref_kmers(const unc_index_t *ix, const char *bwa_prefix, int32_t rid, uint64_t st, uint64_t en, int fwd, uint16_t *out,
                             uint64_t cap, uint64_t *n) {
    if (!ix || !bwa_prefix || !n) return fail(UNC_ERR_ARG, "unc_ref_kmers: null argument");
    if (rid < 0 || rid >= unc_index_n_seqs(ix)) return fail(UNC_ERR_ARG, "unc_ref_kmers: no sequence %d", rid);
    const uint64_t len = unc_index_seq_len(ix, rid);
    if (st > en || en > len) return fail(UNC_ERR_ARG, "unc_ref_kmers: [%llu, %llu) is not inside the sequence's %llu bases",
                                         (unsigned long long)st, (unsigned long long)en, (unsigned long long)len);
    const uint64_t count = en - st >= UNC_KLEN ? en - st - (UNC_KLEN - 1) : 0;
    *n = count;
    if (!out || count == 0) return UNC_OK;
    if (cap < count) return fail(UNC_ERR_ARG, "unc_ref_kmers: room for %llu k-mers is needed", (unsigned long long)count);
    uint64_t offset = 0;        // bntann1_t::offset: the sequences lie one after the other in the packed text
    for (int32_t r = 0; r < rid; ++r) offset += unc_index_seq_len(ix, r);
    const uint64_t a = offset + st, b = offset + en;
    // seq_to_kmers, bp.hpp:125-146: bytes [a >> 2, (b >> 2) + 1) of the .pac, four bases a byte, the first base in the top bits; of
    // the last byte only the b & 3 leading bases (none when b is a multiple of four: the byte is then not read here)
    const uint64_t pst = a >> 2, pen = (b >> 2) + ((b & 3) ? 1 : 0);
    std::vector<uint8_t> pac(pen - pst);
    const std::string fn = std::string(bwa_prefix) + ".pac";
    FILE *fp = fopen(fn.c_str(), "rb");
    if (!fp) return fail(UNC_ERR_IO, "cannot read %s", fn.c_str());
    const bool ok = fseek(fp, (long)pst, SEEK_SET) == 0 && fread(pac.data(), 1, pac.size(), fp) == pac.size();
    fclose(fp);
    if (!ok) return fail(UNC_ERR_IO, "%s too short", fn.c_str());
    uint64_t got = 0, seen = 0;
    uint16_t kmer = 0;
    for (uint64_t pos = a; pos < b; ++pos) {
        const uint8_t base = (pac[(pos >> 2) - pst] >> (((pos & 3) ^ 3) << 1)) & 3;
        kmer = (uint16_t)(((kmer << 2) & (UNC_NKMER - 1)) | base);            // kmer_neighbor, bp.hpp:106-109
        if (++seen >= UNC_KLEN) out[got++] = kmer;
    }
    if (!fwd) {     // kmers_revcomp, bp.hpp:82-99: reversed order, each k-mer reverse-complemented
        std::reverse(out, out + got);
        for (uint64_t i = 0; i < got; ++i) {
            uint16_t r = (uint16_t)~out[i];
            r = (uint16_t)(((r >> 2) & 0x3333) | ((r & 0x3333) << 2));
            r = (uint16_t)(((r >> 4) & 0x0F0F) | ((r & 0x0F0F) << 4));
            r = (uint16_t)(((r >> 8) & 0x00FF) | ((r & 0x00FF) << 8));
            out[i] = (uint16_t)(r >> (2 * (8 - UNC_KLEN)));
        }
    }
    return UNC_OK;
}
