// Host side of the training accumulator (include/uncalled_hip.h: unc_model_acc_*): the launches of k_model_accum (k_model.hip) over
// the caller's arrays, what the alignment (unc_align.cpp) needs of an accumulator, and the exact finish of an accumulator into a
// model.  Compiled as part of unc_align.cpp, which includes this file.
#include <hip/hip_runtime.h>

#include <math.h>
#include <string.h>

#include <vector>

#include "model_dev.h"
#include "unc_host_util.h"
#include "unc_model.h"

using namespace unc;

struct unc_model_acc {
    int device = 0;
    uint32_t flags = 0;
    DevBuf<unsigned long long> d_acc;       // MODEL_ACC_WORDS (model_dev.h)
};

static thread_local float g_model_acc_ms = 0;

extern "C" int unc_model_acc_last_timing(float *ms) {
    if (!ms) return fail(UNC_ERR_ARG, "unc_model_acc_last_timing: null argument");
    *ms = g_model_acc_ms;
    return UNC_OK;
}

namespace unc {
// for the alignment (unc_align.cpp)
void model_acc_set_timing(float ms) { g_model_acc_ms = ms; }
int model_acc_device(const unc_model_acc *acc) { return acc->device; }
void model_acc_args(unc_model_acc *acc, ModelAccum *a) { a->acc = acc->d_acc.p; a->flags = acc->flags; }
}  // namespace unc

extern "C" int unc_model_acc_create(int device, uint32_t flags, unc_model_acc_t **out) {
    if (!out) return fail(UNC_ERR_ARG, "unc_model_acc_create: null argument");
    *out = nullptr;
    if (device < 0 || device >= DTW_MAX_DEVICES) return fail(UNC_ERR_ARG, "unc_model_acc_create: device %d", device);
    if (flags & ~UNC_MODEL_KEEP_SHARED) return fail(UNC_ERR_ARG, "unc_model_acc_create: unknown flags %#x", flags);
    HIPCHK(hipSetDevice(device));
    unc_model_acc *acc = new unc_model_acc();
    struct Guard { unc_model_acc *p; ~Guard() { delete p; } } guard{acc};
    acc->device = device;
    acc->flags = flags;
    HIPCHK(acc->d_acc.alloc(MODEL_ACC_WORDS));
    HIPCHK(hipMemset(acc->d_acc.p, 0, MODEL_ACC_WORDS * sizeof(unsigned long long)));
    guard.p = nullptr;
    *out = acc;
    return UNC_OK;
}

extern "C" void unc_model_acc_free(unc_model_acc_t *acc) {
    if (acc) (void)hipSetDevice(acc->device);
    delete acc;
}

extern "C" int unc_model_acc_reset(unc_model_acc_t *acc) {
    if (!acc) return fail(UNC_ERR_ARG, "unc_model_acc_reset: null argument");
    HIPCHK(hipSetDevice(acc->device));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemset(acc->d_acc.p, 0, MODEL_ACC_WORDS * sizeof(unsigned long long)));
    return UNC_OK;
}

extern "C" int unc_model_acc_add(unc_model_acc_t *acc, uint64_t n, const uint16_t *kmers, const float *levels, const uint32_t *shared,
                                 void *stream) {
    if (!acc || (n && (!kmers || !levels))) return fail(UNC_ERR_ARG, "unc_model_acc_add: null argument");
    if (n >= (1ull << 40)) return fail(UNC_ERR_ARG, "unc_model_acc_add: 2^40 or more records in one call");
    for (uint64_t i = 0; i < n; ++i)
        if (kmers[i] >= UNC_NKMER) return fail(UNC_ERR_ARG, "unc_model_acc_add: k-mer %u at %llu is not below %d", kmers[i], (unsigned long long)i, UNC_NKMER);
    g_model_acc_ms = 0;
    if (n == 0) return UNC_OK;
    HIPCHK(hipSetDevice(acc->device));
    hipStream_t st = (hipStream_t)stream;
    DevBuf<uint16_t> d_kmers;
    DevBuf<float> d_levels;
    DevBuf<uint32_t> d_shared;
    DevEvents ev;
    HIPCHK(d_kmers.alloc(n)); HIPCHK(d_levels.alloc(n));
    HIPCHK(hipMemcpyAsync(d_kmers.p, kmers, n * sizeof(uint16_t), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_levels.p, levels, n * sizeof(float), hipMemcpyHostToDevice, st));
    if (shared) {
        HIPCHK(d_shared.alloc(n));
        HIPCHK(hipMemcpyAsync(d_shared.p, shared, n * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    }
    HIPCHK(ev.create(2));
    ModelAccum a{};
    a.acc = acc->d_acc.p; a.flags = acc->flags;
    a.n = n; a.kmers = d_kmers.p; a.levels = d_levels.p; a.shared = shared ? d_shared.p : nullptr;
    HIPCHK(ev.record(0, st));
    launch_model_accum(a, n, st);
    HIPCHK(hipGetLastError());
    HIPCHK(ev.record(1, st));
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(ev.elapsed(0, 1, &g_model_acc_ms));
    return UNC_OK;
}

extern "C" int unc_model_acc_read(const unc_model_acc_t *acc, uint64_t *n1024, int64_t *S1024, uint64_t *SS_lo1024, uint64_t *SS_hi1024,
                                  uint64_t *n_dropped) {
    if (!acc) return fail(UNC_ERR_ARG, "unc_model_acc_read: null argument");
    HIPCHK(hipSetDevice(acc->device));
    std::vector<unsigned long long> h(MODEL_ACC_WORDS);
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(h.data(), acc->d_acc.p, MODEL_ACC_WORDS * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    if (n1024) memcpy(n1024, h.data() + MODEL_ACC_N, UNC_NKMER * 8);
    if (S1024) memcpy(S1024, h.data() + MODEL_ACC_S, UNC_NKMER * 8);
    if (SS_lo1024) memcpy(SS_lo1024, h.data() + MODEL_ACC_LO, UNC_NKMER * 8);
    if (SS_hi1024) memcpy(SS_hi1024, h.data() + MODEL_ACC_HI, UNC_NKMER * 8);
    if (n_dropped) *n_dropped = h[MODEL_ACC_DROPPED];
    return UNC_OK;
}

extern "C" int unc_model_acc_finish(const unc_model_acc_t *acc, const unc_model_t *prior, uint32_t min_obs, unc_model_t **out,
                                    uint32_t *n_kept_prior) {
    if (!acc || !out) return fail(UNC_ERR_ARG, "unc_model_acc_finish: null argument");
    *out = nullptr;
    std::vector<uint64_t> n(UNC_NKMER), lo(UNC_NKMER), hi(UNC_NKMER);
    std::vector<int64_t> S(UNC_NKMER);
    if (int rc = unc_model_acc_read(acc, n.data(), S.data(), lo.data(), hi.data(), nullptr)) return rc;
    float pairs[2 * UNC_NKMER];
    if (prior) memcpy(pairs, prior->pairs, sizeof pairs);
    else model_default_pairs(pairs);
    static_assert(SUMS_Q_ONE == MODEL_Q_ONE, "the finish divides by the scale the kernel multiplies with");
    const uint64_t need = min_obs > 2 ? min_obs : 2;
    uint32_t kept = 0;
    for (uint32_t k = 0; k < (uint32_t)UNC_NKMER; ++k) {
        u128 V = 0;
        if (!sums_variance(n[k], S[k], lo[k], hi[k], &V)) return fail(UNC_ERR_ARG, "unc_model_acc_finish: k-mer %u: n * SS leaves 128 bits", k);
        if (n[k] < need || V == 0) { ++kept; continue; }
        pairs[2 * k] = (float)sums_mean(n[k], S[k]);
        pairs[2 * k + 1] = (float)sums_sd(n[k], V);
    }
    if (n_kept_prior) *n_kept_prior = kept;
    return unc_model_from_pairs(pairs, out);
}
