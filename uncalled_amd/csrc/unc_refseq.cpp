// Host side of the packed reference (include/uncalled_hip.h: unc_refseq_*, unc_align_ref_batch): BwaIndex::load_pacseq
// (bwa_index.hpp) once per run, the checks of a batch of stretches, their cut into runs for k_ref_kmers (k_refseq.hip) and
// unc_align_ref_batch, the second caller of align_run (unc_align.cpp): the call's record (AlignCall, align_dev.h) as unc_align_batch
// fills it, and rows that k_ref_kmers makes from coordinates.  Compiled as part of unc_align.cpp, which includes this file.
#include <hip/hip_runtime.h>

#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "align_dev.h"
#include "refseq_dev.h"
#include "unc_host_util.h"

using namespace unc;

struct unc_refseq {
    int device = 0;
    uint64_t l_pac = 0;
    std::vector<uint64_t> seq_off;       // bntann1_t::offset of every sequence, and l_pac behind the last
    std::vector<uint8_t> pac;            // the file's base bytes
    DevBuf<uint32_t> d_pac;              // the same, and REF_PAC_SLACK_WORDS zeroed words behind the last word that holds a base
    uint64_t device_bytes = 0;
    uint32_t max_blocks = 0;             // of a k_ref_kmers launch
};

static thread_local float g_ref_kmers_ms = 0;

extern "C" int unc_align_ref_last_timing(float *ms_kmers) {
    if (!ms_kmers) return fail(UNC_ERR_ARG, "unc_align_ref_last_timing: null argument");
    *ms_kmers = g_ref_kmers_ms;
    return UNC_OK;
}

extern "C" void unc_refseq_free(unc_refseq_t *rs) { delete rs; }
extern "C" uint64_t unc_refseq_device_bytes(const unc_refseq_t *rs) { return rs ? rs->device_bytes : 0; }

extern "C" int unc_refseq_load(const unc_index_t *ix, const char *bwa_prefix, unc_refseq_t **out) {
    if (!ix || !bwa_prefix || !out) return fail(UNC_ERR_ARG, "unc_refseq_load: null argument");
    *out = nullptr;
    const std::string fn = std::string(bwa_prefix) + ".pac";
    const uint64_t l_pac = unc_index_size(ix) / 2;
    // the layout bwa writes (and uncalled_amd/build_index.py): four bases a byte, a zero byte more where l_pac is a multiple of
    // four, then l_pac % 4
    const uint64_t n_base = (l_pac + 3) / 4, want = l_pac / 4 + 2;
    FILE *fp = fopen(fn.c_str(), "rb");
    if (!fp) return fail(UNC_ERR_IO, "cannot read %s", fn.c_str());
    std::vector<uint8_t> file((size_t)want + 1);       // (one byte more than expected shows a longer file)
    const size_t got = fread(file.data(), 1, file.size(), fp);
    fclose(fp);
    if (got != want) return fail(UNC_ERR_IO, "%s: %s than the %llu bytes of an index of %llu bases", fn.c_str(), got < want ? "shorter" : "longer",
                                 (unsigned long long)want, (unsigned long long)l_pac);
    if (file[(size_t)want - 1] != (uint8_t)(l_pac % 4))
        return fail(UNC_ERR_IO, "%s: the last byte is %u, not l_pac %% 4 = %u", fn.c_str(), file[(size_t)want - 1], (unsigned)(l_pac % 4));
    unc_refseq *rs = new unc_refseq();
    struct Guard { unc_refseq *p; ~Guard() { delete p; } } guard{rs};
    rs->device = index_device(ix);
    rs->l_pac = l_pac;
    const int32_t n_seqs = unc_index_n_seqs(ix);
    rs->seq_off.assign((size_t)n_seqs + 1, 0);
    for (int32_t r = 0; r < n_seqs; ++r) rs->seq_off[(size_t)r + 1] = rs->seq_off[r] + unc_index_seq_len(ix, r);
    if (rs->seq_off.back() != l_pac) return fail(UNC_ERR_IO, "%s: the index's sequences hold %llu bases, the packed text %llu", fn.c_str(),
                                                 (unsigned long long)rs->seq_off.back(), (unsigned long long)l_pac);
    file.resize((size_t)n_base);
    rs->pac.swap(file);
    const size_t words = (size_t)((n_base + 3) / 4) + REF_PAC_SLACK_WORDS;
    HIPCHK(hipSetDevice(rs->device));
    HIPCHK(rs->d_pac.alloc(words));
    HIPCHK(hipMemset(rs->d_pac.p, 0, words * sizeof(uint32_t)));
    HIPCHK(hipMemcpy(rs->d_pac.p, rs->pac.data(), (size_t)n_base, hipMemcpyHostToDevice));
    rs->device_bytes = words * sizeof(uint32_t);
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, rs->device));
    rs->max_blocks = 4u * (uint32_t)std::max(1, prop.multiProcessorCount);
    guard.p = nullptr;
    *out = rs;
    return UNC_OK;
}

namespace {
// a stretch's first base in the packed text and its k-mers; `what` a names the stretch in the message
int locate_stretch(const unc_refseq *rs, const char *who, const char *what, uint32_t a, const unc_ref_stretch_t &s, uint64_t *base, uint64_t *n) {
    if (s.rid < 0 || (size_t)s.rid + 1 >= rs->seq_off.size()) return fail(UNC_ERR_ARG, "%s: %s %u: no sequence %d", who, what, a, s.rid);
    const uint64_t len = rs->seq_off[(size_t)s.rid + 1] - rs->seq_off[s.rid];
    if (s.st > s.en || s.en > len) return fail(UNC_ERR_ARG, "%s: %s %u: [%llu, %llu) is not inside the sequence's %llu bases", who, what, a,
                                               (unsigned long long)s.st, (unsigned long long)s.en, (unsigned long long)len);
    *base = rs->seq_off[s.rid] + s.st;
    *n = s.en - s.st >= UNC_KLEN ? s.en - s.st - (UNC_KLEN - 1) : 0;
    return UNC_OK;
}

// one wavefront's work each: n k-mers from `base` on, to the elements from out_off on of an array that begins at a 16-byte boundary.
// The first run ends where the output reaches a multiple of 1024 elements, so that every later run starts aligned
void cut_runs(std::vector<RefKmerRun> &runs, uint64_t base, uint64_t n, bool fwd, uint64_t out_off) {
    constexpr uint64_t RUN = 64ull * REF_KMERS_PER_LANE;
    for (uint64_t lo = 0; lo < n;) {
        const uint64_t hi = std::min<uint64_t>(n, lo + RUN - ((out_off + lo) & 7));
        RefKmerRun r;
        r.pac_bit = 2 * (fwd ? base + lo : base + (n - hi));
        r.out_off = out_off + lo;
        r.n = (uint32_t)(hi - lo);
        r.fwd = fwd ? 1u : 0u;
        runs.push_back(r);
        lo = hi;
    }
}
}  // namespace

extern "C" int unc_refseq_kmers_batch(const unc_refseq_t *rs, uint32_t n, const unc_ref_stretch_t *stretches, uint16_t *out,
                                      const uint64_t *out_off, void *stream) {
    static const char *who = "unc_refseq_kmers_batch";
    if (!rs) return fail(UNC_ERR_ARG, "%s: null argument", who);
    if (n == 0) return UNC_OK;
    if (!stretches || !out || !out_off) return fail(UNC_ERR_ARG, "%s: null argument", who);
    // the device array mirrors out[out_off[0] .. out_off[n]): a stretch lies there as it lies in the caller's array
    std::vector<RefKmerRun> runs;
    std::vector<uint64_t> count(n);
    for (uint32_t a = 0; a < n; ++a) {
        uint64_t base = 0;
        if (int rc = locate_stretch(rs, who, "stretch", a, stretches[a], &base, &count[a])) return rc;
        if (out_off[a + 1] < out_off[a]) return fail(UNC_ERR_ARG, "%s: out_off must ascend", who);
        if (out_off[a + 1] - out_off[a] < count[a]) return fail(UNC_ERR_ARG, "%s: stretch %u: room for %llu k-mers is needed", who, a,
                                                                (unsigned long long)count[a]);
        cut_runs(runs, base, count[a], stretches[a].fwd != 0, out_off[a] - out_off[0]);
    }
    if (runs.empty()) return UNC_OK;
    if (runs.size() >= (1ull << 32)) return fail(UNC_ERR_ARG, "%s: 2^42 or more k-mers in one call", who);
    const uint64_t total = out_off[n] - out_off[0];

    HIPCHK(hipSetDevice(rs->device));
    hipStream_t st = (hipStream_t)stream;
    DevBuf<RefKmerRun> d_runs;
    DevBuf<uint16_t> d_out;
    HIPCHK(d_runs.alloc(runs.size())); HIPCHK(d_out.alloc(total));
    HIPCHK(hipMemcpyAsync(d_runs.p, runs.data(), runs.size() * sizeof(RefKmerRun), hipMemcpyHostToDevice, st));
    launch_ref_kmers(rs->d_pac.p, d_runs.p, (uint32_t)runs.size(), d_out.p, rs->max_blocks, st);
    HIPCHK(hipGetLastError());
    // (what lies between the stretches on the device was never written: only the counts are dealt out)
    HIPCHK(deal_out(d_out.p, (size_t)total, st, n, [&](uint32_t a) { return count[a]; }, [&](uint32_t a) { return out_off[a] - out_off[0]; },
                    [&](uint32_t a) { return out + out_off[a]; }));
    return UNC_OK;
}

// ------------------------------------------------------------------ unc_align_ref_batch: the rows made on the device from coordinates
namespace {
struct GeneratedRows : AlignRows {
    const unc_refseq *rs;
    const unc_ref_stretch_t *stretches;
    const uint64_t *kmers_off;           // null without the tap
    std::vector<RefKmerRun> runs;
    std::vector<uint64_t> at;            // first element of every query's rows on the device: a multiple of 8
    std::vector<uint32_t> count;
    uint64_t total = 0;
    DevBuf<uint16_t> d_kmers;
    DevBuf<RefKmerRun> d_runs;
    DevEvents ev;                        // (timing only) around k_ref_kmers
    GeneratedRows(const unc_refseq *r, const unc_ref_stretch_t *s, const uint64_t *off) : rs(r), stretches(s), kmers_off(off) {}
    int rows(uint32_t q, uint64_t *where, uint32_t *n) override {
        static const char *who = "unc_align_ref_batch";
        uint64_t base = 0, cnt = 0;
        if (int rc = locate_stretch(rs, who, "query", q, stretches[q], &base, &cnt)) return rc;
        if (cnt == 0) return fail(UNC_ERR_ARG, "%s: query %u has no k-mers", who, q);
        if (cnt >= (1ull << 31)) return fail(UNC_ERR_ARG, "%s: query %u: 2^31 or more k-mers", who, q);
        if (kmers_off && kmers_off[q + 1] < kmers_off[q]) return fail(UNC_ERR_ARG, "%s: kmers_off must ascend", who);
        if (kmers_off && kmers_off[q + 1] - kmers_off[q] < cnt) return fail(UNC_ERR_ARG, "%s: query %u: room for %llu k-mers is needed", who, q,
                                                                          (unsigned long long)cnt);
        cut_runs(runs, base, cnt, stretches[q].fwd != 0, total);
        at.push_back(total);
        count.push_back((uint32_t)cnt);
        *where = total;
        *n = (uint32_t)cnt;
        total = (total + cnt + 7) & ~7ull;
        return UNC_OK;
    }
    int check() override {
        if (runs.size() >= (1ull << 32)) return fail(UNC_ERR_ARG, "unc_align_ref_batch: 2^42 or more k-mers in one call");
        return UNC_OK;
    }
    int queue(hipStream_t st, const uint16_t **out) override {
        HIPCHK(d_kmers.alloc(total)); HIPCHK(d_runs.alloc(runs.size()));
        HIPCHK(ev.create(2));
        HIPCHK(hipMemcpyAsync(d_runs.p, runs.data(), runs.size() * sizeof(RefKmerRun), hipMemcpyHostToDevice, st));
        HIPCHK(ev.record(0, st));
        launch_ref_kmers(rs->d_pac.p, d_runs.p, (uint32_t)runs.size(), d_kmers.p, rs->max_blocks, st);
        HIPCHK(hipGetLastError());
        HIPCHK(ev.record(1, st));
        *out = d_kmers.p;
        return UNC_OK;
    }
};
}  // namespace

// unc_align_ref_batch, and with c.segs unc_align_ref_segments_batch: the call's record, and what is this route's own
static int align_ref(AlignCall c, const unc_refseq_t *rs, const unc_ref_stretch_t *stretches, uint16_t *kmers_out, const uint64_t *kmers_off) {
    if (!rs || !stretches) return fail(UNC_ERR_ARG, "%s: null argument", c.who);
    if (kmers_out && !kmers_off) return fail(UNC_ERR_ARG, "%s: kmers_out without kmers_off", c.who);
    g_ref_kmers_ms = 0;
    c.device = rs->device;
    GeneratedRows rows(rs, stretches, kmers_out ? kmers_off : nullptr);
    if (int rc = align_run(c, rows)) return rc;
    if (rows.ev.e.empty()) return UNC_OK;    // (no queries: nothing was queued)
    HIPCHK(rows.ev.elapsed(0, 1, &g_ref_kmers_ms));       // (align_run has waited for the stream)
    if (kmers_out)           // the tap: the rows as they lie on the device, dealt out on the host
        HIPCHK(deal_out(rows.d_kmers.p, (size_t)rows.total, (hipStream_t)c.stream, c.n_queries, [&](uint32_t q) { return rows.count[q]; },
                        [&](uint32_t q) { return rows.at[q]; }, [&](uint32_t q) { return kmers_out + kmers_off[q]; }));
    return UNC_OK;
}

extern "C" int unc_align_ref_batch(const unc_refseq_t *rs, const unc_params_t *params, const unc_align_opts_t *opts, uint32_t n_reads,
                                   const int16_t *raw, const uint64_t *offsets, const unc_calib_t *calib, int on_device, uint32_t n_queries,
                                   const unc_align_query_t *queries, const unc_ref_stretch_t *stretches, uint64_t workspace_bytes,
                                   unc_align_result_t *results, float *levels, const uint64_t *lev_off, uint16_t *kmers_out,
                                   const uint64_t *kmers_off, uint32_t *path, const uint64_t *path_off, void *stream) {
    // (the device is the reference's: align_ref sets it once rs is known not to be null)
    unc_align_call_t u = align_record(0, params, opts, n_reads, raw, offsets, calib, on_device, n_queries, queries, workspace_bytes, results,
                                      levels, lev_off, path, path_off, nullptr, stream);
    u.refseq = rs; u.stretches = stretches; u.kmers_out = kmers_out; u.kmers_off = kmers_off;
    if (!rs || !stretches) return fail(UNC_ERR_ARG, "%s: null argument", "unc_align_ref_batch");
    return align_dispatch(u, "unc_align_ref_batch");
}

extern "C" int unc_align_ref_segments_batch(const unc_refseq_t *rs, const unc_params_t *params, const unc_align_opts_t *opts, uint32_t n_reads,
                                            const int16_t *raw, const uint64_t *offsets, const unc_calib_t *calib, int on_device,
                                            uint32_t n_queries, const unc_align_query_t *queries, const unc_ref_stretch_t *stretches,
                                            uint64_t workspace_bytes, unc_align_result_t *results, float *levels, const uint64_t *lev_off,
                                            uint16_t *kmers_out, const uint64_t *kmers_off, uint32_t *path, const uint64_t *path_off,
                                            const unc_align_segments_t *out, void *stream) {
    unc_align_call_t u = align_record(0, params, opts, n_reads, raw, offsets, calib, on_device, n_queries, queries, workspace_bytes, results,
                                      levels, lev_off, path, path_off, out, stream);
    u.refseq = rs; u.stretches = stretches; u.kmers_out = kmers_out; u.kmers_off = kmers_off;
    if (!out || !rs || !stretches) return fail(UNC_ERR_ARG, "%s: null argument", "unc_align_ref_segments_batch");
    return align_dispatch(u, "unc_align_ref_segments_batch");
}
