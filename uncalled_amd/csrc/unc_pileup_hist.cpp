// Host side of the pile-up's level histograms (include/uncalled_hip.h: unc_pileup_hist_*, unc_pileup_ks): attaching one to an empty
// pile-up, reading listed bins' rows and centres, and the two-sample Kolmogorov-Smirnov distance of two pile-ups' rows, whose integer
// part k_pileup_ks (k_pileup_hist.hip) computes and whose two doubles are made here.  What reset, merge, device_bytes and the adds do
// with a histogram is in unc_pileup.cpp.  Compiled as part of unc_align.cpp, which includes this file behind unc_pileup.cpp.
#include <hip/hip_runtime.h>

#include <math.h>
#include <string.h>

#include <cmath>
#include <vector>

#include "model_dev.h"
#include "pileup_dev.h"
#include "unc_host_util.h"
#include "unc_model.h"

using namespace unc;

static thread_local float g_pileup_ks_ms = 0;

extern "C" int unc_pileup_ks_last_timing(float *ms) {
    if (!ms) return fail(UNC_ERR_ARG, "unc_pileup_ks_last_timing: null argument");
    *ms = g_pileup_ks_ms;
    return UNC_OK;
}

extern "C" int unc_pileup_hist_enable(unc_pileup_t *pu, const unc_model_t *model, float width) {
    static const char *who = "unc_pileup_hist_enable";
    if (!pu) return fail(UNC_ERR_ARG, "%s: null argument", who);
    if (pu->hist_w) return fail(UNC_ERR_ARG, "%s: the pile-up has a histogram already", who);
    const double scaled = (double)width * MODEL_Q_ONE;          // exact: a float times a power of two
    if (!std::isfinite(width) || !(scaled >= 0.5 && scaled <= 2147483648.5)) return fail(UNC_ERR_ARG, "%s: a bucket width of %g levels", who, (double)width);
    const long long w = llrint(scaled);
    if (w < 1 || w > (1ll << 31)) return fail(UNC_ERR_ARG, "%s: a bucket width of %g levels", who, (double)width);
    std::vector<float> dflt;
    const float *pairs = model ? model->pairs : nullptr;
    if (!pairs) {
        dflt.resize(2 * UNC_NKMER);
        model_default_pairs(dflt.data());
        pairs = dflt.data();
    }
    std::vector<int64_t> ctab(UNC_NKMER);
    for (uint32_t k = 0; k < (uint32_t)UNC_NKMER; ++k) {
        const float mean = pairs[2 * k];
        if (!std::isfinite(mean) || !(fabsf(mean) < MODEL_LEVEL_LIMIT)) return fail(UNC_ERR_ARG, "%s: the model's mean %g of k-mer %u", who, (double)mean, k);
        ctab[k] = llrint((double)mean * MODEL_Q_ONE);
    }
    if (pu->n_bins >= (1ull << 30)) return fail(UNC_ERR_NOMEM, "%s: a histogram for %llu bins: histograms are meant for regions", who,
                                                (unsigned long long)pu->n_bins);
    // nothing on the device has been allocated or written so far; the counters are read
    uint64_t n_dropped = 0, n_outside = 0, n_added = 0;
    if (int rc = unc_pileup_counters(pu, &n_dropped, &n_outside, &n_added)) return rc;
    if (n_dropped || n_outside || n_added) return fail(UNC_ERR_ARG, "%s: the pile-up holds records: a histogram is attached to an empty one", who);
    HIPCHK(hipSetDevice(pu->device));
    DevBuf<uint32_t> d_hist;
    DevBuf<int64_t> d_centres, d_ctab;
    DevBuf<uint64_t> d_base;
    if (d_hist.alloc(pu->buckets()) != hipSuccess || d_centres.alloc((size_t)pu->n_bins) != hipSuccess) {
        (void)hipGetLastError();
        return fail(UNC_ERR_NOMEM, "%s: no device memory for the histograms of %llu bins (%llu bytes)", who, (unsigned long long)pu->n_bins,
                    (unsigned long long)(pu->buckets() * sizeof(uint32_t) + pu->n_bins * sizeof(int64_t)));
    }
    std::vector<uint64_t> base(pu->regions.size());
    for (size_t r = 0; r < base.size(); ++r) base[r] = pu->rs->seq_off[pu->regions[r].rid] + pu->regions[r].st;
    HIPCHK(d_ctab.alloc(ctab.size())); HIPCHK(d_base.alloc(base.size()));
    HIPCHK(hipMemcpy(d_ctab.p, ctab.data(), ctab.size() * sizeof(int64_t), hipMemcpyHostToDevice));
    if (!base.empty()) HIPCHK(hipMemcpy(d_base.p, base.data(), base.size() * sizeof(uint64_t), hipMemcpyHostToDevice));
    if (pu->buckets()) HIPCHK(hipMemset(d_hist.p, 0, pu->buckets() * sizeof(uint32_t)));
    launch_pileup_hist_centres(pu->rs->d_pac.p, pu->d_regions.p, d_base.p, (uint32_t)pu->regions.size(), pu->n_bins / 2, d_ctab.p, d_centres.p, nullptr);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(nullptr));
    pu->d_hist = std::move(d_hist);
    pu->d_centres = std::move(d_centres);
    pu->hist_ctab.swap(ctab);
    pu->hist_w = w;
    return UNC_OK;
}

extern "C" int unc_pileup_hist_gather(const unc_pileup_t *pu, uint64_t n, const uint64_t *bins, uint32_t *out_counts) {
    static const char *who = "unc_pileup_hist_gather";
    if (!pu || (n && !out_counts)) return fail(UNC_ERR_ARG, "%s: null argument", who);
    if (!pu->hist_w) return fail(UNC_ERR_ARG, "%s: the pile-up has no histogram", who);
    if (int rc = check_bins(pu, who, n, bins)) return rc;
    if (n == 0) return UNC_OK;
    HIPCHK(hipSetDevice(pu->device));
    HIPCHK(hipDeviceSynchronize());
    DevBuf<uint64_t> d_bins;
    DevBuf<uint32_t> d_out;
    HIPCHK(d_bins.alloc(n)); HIPCHK(d_out.alloc(n * PILEUP_HIST_BUCKETS));
    HIPCHK(hipMemcpyAsync(d_bins.p, bins, n * sizeof(uint64_t), hipMemcpyHostToDevice, nullptr));
    launch_pileup_hist_gather(pu->d_hist.p, d_bins.p, n, d_out.p, nullptr);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out_counts, d_out.p, n * PILEUP_HIST_BUCKETS * sizeof(uint32_t), hipMemcpyDeviceToHost, nullptr));
    HIPCHK(hipStreamSynchronize(nullptr));
    return UNC_OK;
}

extern "C" int unc_pileup_hist_centres(const unc_pileup_t *pu, uint64_t n, const uint64_t *bins, int64_t *out_q) {
    static const char *who = "unc_pileup_hist_centres";
    if (!pu || (n && !out_q)) return fail(UNC_ERR_ARG, "%s: null argument", who);
    if (!pu->hist_w) return fail(UNC_ERR_ARG, "%s: the pile-up has no histogram", who);
    if (int rc = check_bins(pu, who, n, bins)) return rc;
    if (n == 0) return UNC_OK;
    HIPCHK(hipSetDevice(pu->device));
    HIPCHK(hipDeviceSynchronize());
    DevBuf<uint64_t> d_bins;
    DevBuf<int64_t> d_out;
    HIPCHK(d_bins.alloc(n)); HIPCHK(d_out.alloc(n));
    HIPCHK(hipMemcpyAsync(d_bins.p, bins, n * sizeof(uint64_t), hipMemcpyHostToDevice, nullptr));
    launch_pileup_centres_gather(pu->d_centres.p, d_bins.p, n, d_out.p, nullptr);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out_q, d_out.p, n * sizeof(int64_t), hipMemcpyDeviceToHost, nullptr));
    HIPCHK(hipStreamSynchronize(nullptr));
    return UNC_OK;
}

extern "C" int unc_pileup_ks(const unc_pileup_t *a, const unc_pileup_t *b, uint64_t n, const uint64_t *bins, unc_pileup_ks_t *out) {
    static const char *who = "unc_pileup_ks";
    static_assert(sizeof(unc_pileup_ks_t) == 48 && sizeof(PileupKs) == 32, "the record of a bin, for the caller and on the device");
    if (!a || !b || (n && !out)) return fail(UNC_ERR_ARG, "%s: null argument", who);
    if (!a->hist_w || !b->hist_w) return fail(UNC_ERR_ARG, "%s: a pile-up without a histogram", who);
    if (a->device != b->device || !same_regions(a, b)) return fail(UNC_ERR_ARG, "%s: the two pile-ups differ in their regions or their device", who);
    if (!same_hist(a, b)) return fail(UNC_ERR_ARG, "%s: the two histograms differ in their bucket width or their centres", who);
    if (n >= (1ull << 32)) return fail(UNC_ERR_ARG, "%s: 2^32 or more bins in one call", who);
    if (int rc = check_bins(a, who, n, bins)) return rc;
    g_pileup_ks_ms = 0;
    if (n == 0) return UNC_OK;
    // the counts from the pile-ups' own words: a bucket's 32 bits may have wrapped where n does not fit them
    std::vector<BinSums> wa, wb;
    if (int rc = fetch_bins(a, n, bins, wa)) return rc;
    if (int rc = fetch_bins(b, n, bins, wb)) return rc;
    for (uint64_t i = 0; i < n; ++i)
        if (wa[i].n == 0 || wb[i].n == 0 || wa[i].n >= (1ull << 32) || wb[i].n >= (1ull << 32))
            return fail(UNC_ERR_ARG, "%s: bin %llu holds %llu and %llu records: 1 to 2^32 - 1 each are needed", who, (unsigned long long)bins[i],
                        (unsigned long long)wa[i].n, (unsigned long long)wb[i].n);
    HIPCHK(hipSetDevice(a->device));
    DevBuf<uint64_t> d_bins;
    DevBuf<PileupKs> d_out;
    DevEvents ev;
    std::vector<PileupKs> h((size_t)n);
    HIPCHK(d_bins.alloc(n)); HIPCHK(d_out.alloc(n));
    HIPCHK(ev.create(2));
    hipStream_t st = nullptr;
    HIPCHK(hipMemcpyAsync(d_bins.p, bins, n * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    HIPCHK(ev.record(0, st));
    launch_pileup_ks(a->d_hist.p, b->d_hist.p, d_bins.p, n, d_out.p, st);
    HIPCHK(hipGetLastError());
    HIPCHK(ev.record(1, st));
    HIPCHK(hipMemcpyAsync(h.data(), d_out.p, n * sizeof(PileupKs), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(ev.elapsed(0, 1, &g_pileup_ks_ms));
    for (uint64_t i = 0; i < n; ++i) {
        unc_pileup_ks_t &o = out[i];
        o.n_a = h[i].n_a; o.n_b = h[i].n_b; o.num = h[i].num; o.bucket = h[i].bucket; o.sign = h[i].sign;
        const double prod = (double)o.n_a * (double)o.n_b;
        const double sum = (double)o.n_a + (double)o.n_b;
        o.d = (double)o.num / prod;
        const double scale = sqrt(prod / sum);
        o.ks = o.d * scale;
    }
    return UNC_OK;
}
