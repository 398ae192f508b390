// Host side of the signal pile-up (include/uncalled_hip.h: unc_pileup_*): the region table and the bins' numbering, the launches of
// k_pileup.hip's kernels, what the alignment (unc_align.cpp) needs of a pile-up, and the exact statistics of listed bins.  Compiled as
// part of unc_align.cpp, which includes this file behind unc_refseq.cpp (the packed reference's struct) and unc_model_acc.cpp.
#include <hip/hip_runtime.h>

#include <math.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "model_dev.h"
#include "pileup_dev.h"
#include "unc_host_util.h"
#include "unc_model.h"

using namespace unc;

struct unc_pileup {
    const unc_refseq *rs = nullptr;
    int device = 0;
    uint32_t flags = 0;
    uint64_t n_bins = 0;
    std::vector<PileupRegion> regions;      // sorted by (rid, st); bin0 ascends
    DevBuf<PileupRegion> d_regions;
    DevBuf<unsigned long long> d_tab;       // PILEUP_WORDS * n_bins words, then PILEUP_COUNTERS
    size_t words() const { return (size_t)(PILEUP_WORDS * n_bins + PILEUP_COUNTERS); }
    // the histogram (unc_pileup_hist.cpp), attached by unc_pileup_hist_enable: hist_w == 0 without one
    int64_t hist_w = 0;
    std::vector<int64_t> hist_ctab;         // the 1024 centres it was attached with, in k-mer order
    DevBuf<uint32_t> d_hist;                // PILEUP_HIST_BUCKETS * n_bins buckets
    DevBuf<int64_t> d_centres;              // n_bins
    size_t buckets() const { return (size_t)(PILEUP_HIST_BUCKETS * n_bins); }
    size_t hist_bytes() const { return hist_w ? std::max<size_t>(1, buckets()) * sizeof(uint32_t) + std::max<size_t>(1, (size_t)n_bins) * sizeof(int64_t) : 0; }
};

static thread_local float g_pileup_ms = 0;
static thread_local float g_pileup_cov_ms[3] = {0, 0, 0};

extern "C" int unc_pileup_last_timing(float *ms) {
    if (!ms) return fail(UNC_ERR_ARG, "unc_pileup_last_timing: null argument");
    *ms = g_pileup_ms;
    return UNC_OK;
}

extern "C" int unc_pileup_covered_last_timing(float *ms3) {
    if (!ms3) return fail(UNC_ERR_ARG, "unc_pileup_covered_last_timing: null argument");
    memcpy(ms3, g_pileup_cov_ms, sizeof g_pileup_cov_ms);
    return UNC_OK;
}

namespace unc {
// for the alignment (unc_align.cpp)
void pileup_set_timing(float ms) { g_pileup_ms = ms; }
int pileup_device(const unc_pileup *pu) { return pu->device; }
const unc_refseq *pileup_refseq(const unc_pileup *pu) { return pu->rs; }
void pileup_args(unc_pileup *pu, PileupAccum *a) {
    a->tab = pu->d_tab.p; a->regions = pu->d_regions.p; a->n_bins = pu->n_bins; a->n_regions = (uint32_t)pu->regions.size(); a->flags = pu->flags;
}
bool pileup_hist_args(unc_pileup *pu, PileupHist *h) {
    h->hist = pu->d_hist.p; h->centres = pu->d_centres.p; h->w = pu->hist_w;
    return pu->hist_w != 0;
}
}  // namespace unc

namespace {
bool same_regions(const unc_pileup *a, const unc_pileup *b) {
    if (a->regions.size() != b->regions.size() || a->n_bins != b->n_bins) return false;
    for (size_t i = 0; i < a->regions.size(); ++i) {
        const PileupRegion &x = a->regions[i], &y = b->regions[i];
        if (x.rid != y.rid || x.st != y.st || x.n != y.n || x.bin0 != y.bin0) return false;
    }
    return true;
}

// both without a histogram, or both with one of the same width and the same 1024 centres
bool same_hist(const unc_pileup *a, const unc_pileup *b) { return a->hist_w == b->hist_w && a->hist_ctab == b->hist_ctab; }

// the region that holds `bin`: the last one whose first bin is not behind it and that holds a bin at all
const PileupRegion *region_of_bin(const unc_pileup *pu, uint64_t bin) {
    const uint64_t at = bin / 2;
    size_t lo = 0, hi = pu->regions.size();
    while (lo < hi) {
        const size_t mid = lo + (hi - lo) / 2;
        if (pu->regions[mid].bin0 + pu->regions[mid].n <= at) lo = mid + 1;
        else hi = mid;
    }
    return lo < pu->regions.size() && pu->regions[lo].bin0 <= at ? &pu->regions[lo] : nullptr;
}

int check_bins(const unc_pileup *pu, const char *who, uint64_t n, const uint64_t *bins) {
    if (n && !bins) return fail(UNC_ERR_ARG, "%s: null argument", who);
    for (uint64_t i = 0; i < n; ++i)
        if (bins[i] >= pu->n_bins) return fail(UNC_ERR_ARG, "%s: bin %llu at %llu is not below %llu", who, (unsigned long long)bins[i],
                                               (unsigned long long)i, (unsigned long long)pu->n_bins);
    return UNC_OK;
}

// the 5-mer whose leftmost base is base g of the packed text (four bases a byte, the first in the top bits), first base most significant
uint32_t host_kmer(const unc_refseq *rs, uint64_t g, bool fwd) {
    uint32_t k = 0, rc = 0;
    for (uint32_t i = 0; i < UNC_KLEN; ++i) {
        const uint64_t at = g + i;
        const uint32_t base = (rs->pac[(size_t)(at >> 2)] >> ((~at & 3u) << 1)) & 3u;
        k = (k << 2) | base;
        rc |= (3u - base) << (2 * i);
    }
    return fwd ? k : rc;
}

struct BinSums { uint64_t n; int64_t S; uint64_t lo, hi, D; };

// the listed bins' words on the host (the gather kernel, then one copy)
int fetch_bins(const unc_pileup *pu, uint64_t n, const uint64_t *bins, std::vector<BinSums> &out) {
    static_assert(sizeof(BinSums) == PILEUP_WORDS * sizeof(uint64_t), "a bin's five words");
    out.resize((size_t)n);
    return n ? unc_pileup_gather(pu, n, bins, (uint64_t *)out.data()) : UNC_OK;
}
}  // namespace

extern "C" int unc_pileup_create(const unc_refseq_t *rs, uint32_t n_regions, const unc_ref_stretch_t *regions, uint32_t flags, unc_pileup_t **out) {
    static const char *who = "unc_pileup_create";
    if (!rs || !out || (n_regions && !regions)) return fail(UNC_ERR_ARG, "%s: null argument", who);
    *out = nullptr;
    if (flags & ~UNC_PILEUP_KEEP_SHARED) return fail(UNC_ERR_ARG, "%s: unknown flags %#x", who, flags);
    const size_t n_seqs = rs->seq_off.size() - 1;
    std::vector<unc_ref_stretch_t> rg;
    if (regions) rg.assign(regions, regions + n_regions);
    else
        for (size_t r = 0; r < n_seqs; ++r) rg.push_back(unc_ref_stretch_t{(int32_t)r, 1u, 0, rs->seq_off[r + 1] - rs->seq_off[r]});
    for (size_t i = 0; i < rg.size(); ++i) {
        const unc_ref_stretch_t &s = rg[i];
        if (s.rid < 0 || (size_t)s.rid >= n_seqs) return fail(UNC_ERR_ARG, "%s: region %zu: no sequence %d", who, i, s.rid);
        const uint64_t len = rs->seq_off[(size_t)s.rid + 1] - rs->seq_off[s.rid];
        if (s.st > s.en || s.en > len) return fail(UNC_ERR_ARG, "%s: region %zu: [%llu, %llu) is not inside the sequence's %llu bases", who, i,
                                                   (unsigned long long)s.st, (unsigned long long)s.en, (unsigned long long)len);
    }
    std::sort(rg.begin(), rg.end(), [](const unc_ref_stretch_t &a, const unc_ref_stretch_t &b) {
        return a.rid != b.rid ? a.rid < b.rid : a.st != b.st ? a.st < b.st : a.en < b.en;
    });
    for (size_t i = 1; i < rg.size(); ++i)
        if (rg[i].rid == rg[i - 1].rid && rg[i - 1].en > rg[i].st)
            return fail(UNC_ERR_ARG, "%s: regions [%llu, %llu) and [%llu, %llu) of sequence %d overlap", who, (unsigned long long)rg[i - 1].st,
                        (unsigned long long)rg[i - 1].en, (unsigned long long)rg[i].st, (unsigned long long)rg[i].en, rg[i].rid);
    unc_pileup *pu = new unc_pileup();
    struct Guard { unc_pileup *p; ~Guard() { delete p; } } guard{pu};
    pu->rs = rs;
    pu->device = rs->device;
    pu->flags = flags;
    uint64_t at = 0;
    for (const unc_ref_stretch_t &s : rg) {
        PileupRegion R{};
        R.st = s.st; R.n = s.en - s.st >= UNC_KLEN ? s.en - s.st - (UNC_KLEN - 1) : 0; R.bin0 = at; R.rid = s.rid;
        pu->regions.push_back(R);
        at += R.n;
    }
    pu->n_bins = 2 * at;
    if (pu->n_bins >= (1ull << 38)) return fail(UNC_ERR_NOMEM, "%s: a table of %llu bins", who, (unsigned long long)pu->n_bins);
    HIPCHK(hipSetDevice(pu->device));
    HIPCHK(pu->d_regions.alloc(pu->regions.size()));
    if (pu->d_tab.alloc(pu->words()) != hipSuccess) {
        (void)hipGetLastError();
        return fail(UNC_ERR_NOMEM, "%s: no device memory for a table of %llu bins (%llu bytes)", who, (unsigned long long)pu->n_bins,
                    (unsigned long long)(pu->words() * 8));
    }
    if (!pu->regions.empty())
        HIPCHK(hipMemcpy(pu->d_regions.p, pu->regions.data(), pu->regions.size() * sizeof(PileupRegion), hipMemcpyHostToDevice));
    HIPCHK(hipMemset(pu->d_tab.p, 0, pu->words() * sizeof(unsigned long long)));
    guard.p = nullptr;
    *out = pu;
    return UNC_OK;
}

extern "C" void unc_pileup_free(unc_pileup_t *pu) {
    if (pu) (void)hipSetDevice(pu->device);
    delete pu;
}

extern "C" int unc_pileup_reset(unc_pileup_t *pu) {
    if (!pu) return fail(UNC_ERR_ARG, "unc_pileup_reset: null argument");
    HIPCHK(hipSetDevice(pu->device));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemset(pu->d_tab.p, 0, pu->words() * sizeof(unsigned long long)));
    if (pu->hist_w && pu->buckets()) HIPCHK(hipMemset(pu->d_hist.p, 0, pu->buckets() * sizeof(uint32_t)));       // (the centres stay)
    return UNC_OK;
}

extern "C" uint64_t unc_pileup_device_bytes(const unc_pileup_t *pu) {
    return pu ? pu->words() * sizeof(unsigned long long) + std::max<size_t>(1, pu->regions.size()) * sizeof(PileupRegion) + pu->hist_bytes() : 0;
}
extern "C" uint64_t unc_pileup_n_bins(const unc_pileup_t *pu) { return pu ? pu->n_bins : 0; }

extern "C" int unc_pileup_counters(const unc_pileup_t *pu, uint64_t *n_dropped, uint64_t *n_outside, uint64_t *n_added) {
    if (!pu) return fail(UNC_ERR_ARG, "unc_pileup_counters: null argument");
    HIPCHK(hipSetDevice(pu->device));
    HIPCHK(hipDeviceSynchronize());
    unsigned long long h[PILEUP_COUNTERS];
    HIPCHK(hipMemcpy(h, pu->d_tab.p + PILEUP_WORDS * pu->n_bins, sizeof h, hipMemcpyDeviceToHost));
    if (n_dropped) *n_dropped = h[PILEUP_DROPPED];
    if (n_outside) *n_outside = h[PILEUP_OUTSIDE];
    if (n_added) *n_added = h[PILEUP_ADDED];
    return UNC_OK;
}

extern "C" int unc_pileup_add(unc_pileup_t *pu, uint64_t n, const int32_t *rid, const uint64_t *pos, const uint32_t *fwd, const float *level,
                              const uint32_t *smp_n, const uint32_t *shared, void *stream) {
    static const char *who = "unc_pileup_add";
    if (!pu || (n && (!rid || !pos || !fwd || !level || !smp_n))) return fail(UNC_ERR_ARG, "%s: null argument", who);
    if (n >= (1ull << 40)) return fail(UNC_ERR_ARG, "%s: 2^40 or more records in one call", who);
    const size_t n_seqs = pu->rs->seq_off.size() - 1;
    for (uint64_t i = 0; i < n; ++i)
        if (rid[i] < 0 || (size_t)rid[i] >= n_seqs) return fail(UNC_ERR_ARG, "%s: record %llu: no sequence %d", who, (unsigned long long)i, rid[i]);
    g_pileup_ms = 0;
    if (n == 0) return UNC_OK;
    HIPCHK(hipSetDevice(pu->device));
    hipStream_t st = (hipStream_t)stream;
    DevBuf<int32_t> d_rid;
    DevBuf<uint64_t> d_pos;
    DevBuf<uint32_t> d_fwd, d_smp, d_shared;
    DevBuf<float> d_level;
    DevEvents ev;
    HIPCHK(d_rid.alloc(n)); HIPCHK(d_pos.alloc(n)); HIPCHK(d_fwd.alloc(n)); HIPCHK(d_level.alloc(n)); HIPCHK(d_smp.alloc(n));
    HIPCHK(hipMemcpyAsync(d_rid.p, rid, n * sizeof(int32_t), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_pos.p, pos, n * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_fwd.p, fwd, n * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_level.p, level, n * sizeof(float), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_smp.p, smp_n, n * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    if (shared) {
        HIPCHK(d_shared.alloc(n));
        HIPCHK(hipMemcpyAsync(d_shared.p, shared, n * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    }
    HIPCHK(ev.create(2));
    PileupAccum a{};
    pileup_args(pu, &a);
    a.n = n; a.rid = d_rid.p; a.pos = d_pos.p; a.fwd = d_fwd.p; a.level = d_level.p; a.smp_n = d_smp.p; a.shared = shared ? d_shared.p : nullptr;
    HIPCHK(ev.record(0, st));
    launch_pileup_accum(a, n, st);
    HIPCHK(hipGetLastError());
    PileupHist h{};
    if (pileup_hist_args(pu, &h)) launch_pileup_hist_accum(a, h, n, st);       // (inside the two events: last_timing covers both)
    HIPCHK(hipGetLastError());
    HIPCHK(ev.record(1, st));
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(ev.elapsed(0, 1, &g_pileup_ms));
    return UNC_OK;
}

extern "C" int unc_pileup_covered(const unc_pileup_t *a, const unc_pileup_t *b, uint64_t min_cov, uint64_t *bins_out, uint64_t cap, uint64_t *n_out) {
    static const char *who = "unc_pileup_covered";
    if (!a || !n_out || (cap && !bins_out)) return fail(UNC_ERR_ARG, "%s: null argument", who);
    if (min_cov == 0) return fail(UNC_ERR_ARG, "%s: min_cov 0 would list every bin", who);
    if (b && (b->device != a->device || !same_regions(a, b))) return fail(UNC_ERR_ARG, "%s: the two pile-ups differ in their regions or their device", who);
    memset(g_pileup_cov_ms, 0, sizeof g_pileup_cov_ms);
    *n_out = 0;
    if (a->n_bins == 0) return UNC_OK;
    HIPCHK(hipSetDevice(a->device));
    HIPCHK(hipDeviceSynchronize());
    const uint64_t n_blocks = pileup_scan_blocks(a->n_bins);
    DevBuf<uint32_t> d_counts;
    DevBuf<uint64_t> d_offsets, d_out;
    DevEvents ev;
    HIPCHK(d_counts.alloc(n_blocks)); HIPCHK(d_offsets.alloc(n_blocks + 1));
    HIPCHK(ev.create(5));
    hipStream_t st = nullptr;
    HIPCHK(ev.record(0, st));
    launch_pileup_count(a->d_tab.p, b ? b->d_tab.p : nullptr, a->n_bins, min_cov, d_counts.p, st);
    HIPCHK(hipGetLastError());
    HIPCHK(ev.record(1, st));
    launch_pileup_scan(d_counts.p, n_blocks, d_offsets.p, st);
    HIPCHK(hipGetLastError());
    HIPCHK(ev.record(2, st));
    uint64_t total = 0;
    HIPCHK(hipMemcpyAsync(&total, d_offsets.p + n_blocks, sizeof total, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    for (int i = 0; i < 2; ++i) HIPCHK(ev.elapsed(i, i + 1, &g_pileup_cov_ms[i]));
    *n_out = total;
    const uint64_t got = std::min(cap, total);
    if (got == 0) return UNC_OK;
    HIPCHK(d_out.alloc(got));
    HIPCHK(ev.record(3, st));
    launch_pileup_write(a->d_tab.p, b ? b->d_tab.p : nullptr, a->n_bins, min_cov, d_offsets.p, d_out.p, got, st);
    HIPCHK(hipGetLastError());
    HIPCHK(ev.record(4, st));
    HIPCHK(hipMemcpyAsync(bins_out, d_out.p, got * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(ev.elapsed(3, 4, &g_pileup_cov_ms[2]));
    return UNC_OK;
}

extern "C" int unc_pileup_gather(const unc_pileup_t *pu, uint64_t n, const uint64_t *bins, uint64_t *out_words) {
    static const char *who = "unc_pileup_gather";
    if (!pu || (n && !out_words)) return fail(UNC_ERR_ARG, "%s: null argument", who);
    if (int rc = check_bins(pu, who, n, bins)) return rc;
    if (n == 0) return UNC_OK;
    HIPCHK(hipSetDevice(pu->device));
    HIPCHK(hipDeviceSynchronize());
    DevBuf<uint64_t> d_bins;
    DevBuf<unsigned long long> d_out;
    HIPCHK(d_bins.alloc(n)); HIPCHK(d_out.alloc(n * PILEUP_WORDS));
    HIPCHK(hipMemcpyAsync(d_bins.p, bins, n * sizeof(uint64_t), hipMemcpyHostToDevice, nullptr));
    launch_pileup_gather(pu->d_tab.p, d_bins.p, n, d_out.p, nullptr);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out_words, d_out.p, n * PILEUP_WORDS * sizeof(uint64_t), hipMemcpyDeviceToHost, nullptr));
    HIPCHK(hipStreamSynchronize(nullptr));
    return UNC_OK;
}

extern "C" int unc_pileup_bin_locate(const unc_pileup_t *pu, uint64_t n, const uint64_t *bins, int32_t *rid, uint64_t *pos, uint32_t *fwd) {
    static const char *who = "unc_pileup_bin_locate";
    if (!pu) return fail(UNC_ERR_ARG, "%s: null argument", who);
    if (int rc = check_bins(pu, who, n, bins)) return rc;
    for (uint64_t i = 0; i < n; ++i) {
        const PileupRegion *R = region_of_bin(pu, bins[i]);
        if (!R) return fail(UNC_ERR_ARG, "%s: bin %llu lies in no region", who, (unsigned long long)bins[i]);       // (cannot happen)
        if (rid) rid[i] = R->rid;
        if (pos) pos[i] = R->st + (bins[i] / 2 - R->bin0);
        if (fwd) fwd[i] = bins[i] & 1 ? 0u : 1u;
    }
    return UNC_OK;
}

extern "C" int unc_pileup_merge(unc_pileup_t *dst, const unc_pileup_t *src) {
    static const char *who = "unc_pileup_merge";
    if (!dst || !src) return fail(UNC_ERR_ARG, "%s: null argument", who);
    if (dst == src) return fail(UNC_ERR_ARG, "%s: a pile-up cannot be merged into itself", who);
    if (!same_regions(dst, src)) return fail(UNC_ERR_ARG, "%s: the two pile-ups differ in their regions", who);
    if (!same_hist(dst, src)) return fail(UNC_ERR_ARG, "%s: the two pile-ups differ in their histograms: one has none, or the widths or the centres differ", who);
    DevBuf<unsigned long long> staged;
    DevBuf<uint32_t> staged_hist;
    const unsigned long long *d_src = src->d_tab.p;
    const uint32_t *d_src_hist = src->d_hist.p;
    if (src->device != dst->device && src->hist_w && src->buckets()) {
        std::vector<uint32_t> h(src->buckets());
        HIPCHK(hipSetDevice(src->device));
        HIPCHK(hipDeviceSynchronize());
        HIPCHK(hipMemcpy(h.data(), src->d_hist.p, h.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
        HIPCHK(hipSetDevice(dst->device));
        if (staged_hist.alloc(h.size()) != hipSuccess) {
            (void)hipGetLastError();
            return fail(UNC_ERR_NOMEM, "%s: no device memory for the other device's histogram", who);
        }
        HIPCHK(hipMemcpy(staged_hist.p, h.data(), h.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
        d_src_hist = staged_hist.p;
    }
    if (src->device != dst->device) {       // through the host: no peer access is assumed
        std::vector<unsigned long long> h(src->words());
        HIPCHK(hipSetDevice(src->device));
        HIPCHK(hipDeviceSynchronize());
        HIPCHK(hipMemcpy(h.data(), src->d_tab.p, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        HIPCHK(hipSetDevice(dst->device));
        if (staged.alloc(h.size()) != hipSuccess) {
            (void)hipGetLastError();
            return fail(UNC_ERR_NOMEM, "%s: no device memory for the other device's table", who);
        }
        HIPCHK(hipMemcpy(staged.p, h.data(), h.size() * sizeof(unsigned long long), hipMemcpyHostToDevice));
        d_src = staged.p;
    }
    HIPCHK(hipSetDevice(dst->device));
    HIPCHK(hipDeviceSynchronize());
    launch_pileup_merge(dst->d_tab.p, d_src, dst->n_bins, nullptr);
    HIPCHK(hipGetLastError());
    if (dst->hist_w) launch_pileup_hist_merge(dst->d_hist.p, d_src_hist, dst->n_bins, nullptr);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(nullptr));
    return UNC_OK;
}

extern "C" int unc_pileup_stats(const unc_pileup_t *pu, const unc_model_t *model, uint64_t n, const uint64_t *bins, unc_pileup_stat_t *out) {
    static const char *who = "unc_pileup_stats";
    static_assert(SUMS_Q_ONE == MODEL_Q_ONE, "the statistics divide by the scale the kernel multiplies with");
    if (!pu || (n && !out)) return fail(UNC_ERR_ARG, "%s: null argument", who);
    if (int rc = check_bins(pu, who, n, bins)) return rc;
    std::vector<float> dflt;
    const float *pairs = model ? model->pairs : nullptr;
    if (!pairs) {
        dflt.resize(2 * UNC_NKMER);
        model_default_pairs(dflt.data());
        pairs = dflt.data();
    }
    std::vector<BinSums> w;
    if (int rc = fetch_bins(pu, n, bins, w)) return rc;
    for (uint64_t i = 0; i < n; ++i) {
        const PileupRegion *R = region_of_bin(pu, bins[i]);
        if (!R) return fail(UNC_ERR_ARG, "%s: bin %llu lies in no region", who, (unsigned long long)bins[i]);       // (cannot happen)
        const uint64_t p = R->st + (bins[i] / 2 - R->bin0);
        unc_pileup_stat_t &o = out[i];
        memset(&o, 0, sizeof o);
        o.kmer = host_kmer(pu->rs, pu->rs->seq_off[R->rid] + p, !(bins[i] & 1));
        o.model_mean = pairs[2 * o.kmer];
        o.model_stdv = pairs[2 * o.kmer + 1];
        o.n = w[i].n;
        if (o.n == 0) continue;
        u128 V = 0;
        if (!sums_variance(w[i].n, w[i].S, w[i].lo, w[i].hi, &V)) return fail(UNC_ERR_ARG, "%s: bin %llu: n * SS leaves 128 bits", who,
                                                                              (unsigned long long)bins[i]);
        o.mean = sums_mean(w[i].n, w[i].S);
        o.sd = sums_sd(w[i].n, V);
        o.dwell = (double)w[i].D / (double)w[i].n;
        double z = o.mean - (double)o.model_mean;
        z = z / (double)o.model_stdv;
        z = z * sqrt((double)w[i].n);
        o.z = z;
    }
    return UNC_OK;
}

extern "C" int unc_pileup_compare(const unc_pileup_t *a, const unc_pileup_t *b, uint64_t n, const uint64_t *bins, unc_pileup_cmp_t *out) {
    static const char *who = "unc_pileup_compare";
    if (!a || !b || (n && !out)) return fail(UNC_ERR_ARG, "%s: null argument", who);
    if (!same_regions(a, b)) return fail(UNC_ERR_ARG, "%s: the two pile-ups differ in their regions", who);
    if (int rc = check_bins(a, who, n, bins)) return rc;
    std::vector<BinSums> wa, wb;
    if (int rc = fetch_bins(a, n, bins, wa)) return rc;
    if (int rc = fetch_bins(b, n, bins, wb)) return rc;
    for (uint64_t i = 0; i < n; ++i)
        if (wa[i].n < 2 || wb[i].n < 2) return fail(UNC_ERR_ARG, "%s: bin %llu holds %llu and %llu records: two each are needed", who,
                                                    (unsigned long long)bins[i], (unsigned long long)wa[i].n, (unsigned long long)wb[i].n);
    for (uint64_t i = 0; i < n; ++i) {
        u128 Va = 0, Vb = 0;
        if (!sums_variance(wa[i].n, wa[i].S, wa[i].lo, wa[i].hi, &Va) || !sums_variance(wb[i].n, wb[i].S, wb[i].lo, wb[i].hi, &Vb))
            return fail(UNC_ERR_ARG, "%s: bin %llu: n * SS leaves 128 bits", who, (unsigned long long)bins[i]);
        unc_pileup_cmp_t &o = out[i];
        o.n_a = wa[i].n; o.n_b = wb[i].n;
        o.mean_a = sums_mean(wa[i].n, wa[i].S); o.mean_b = sums_mean(wb[i].n, wb[i].S);
        o.sd_a = sums_sd(wa[i].n, Va); o.sd_b = sums_sd(wb[i].n, Vb);
        double ta = o.sd_a * o.sd_a;
        ta = ta / (double)(o.n_a - 1);
        double tb = o.sd_b * o.sd_b;
        tb = tb / (double)(o.n_b - 1);
        o.se2 = ta + tb;
        o.t = 0;
        if (o.se2 > 0) {
            const double d = o.mean_a - o.mean_b;
            o.t = d / sqrt(o.se2);
        }
    }
    return UNC_OK;
}
