// The pore model behind the C ABI (include/uncalled_hip.h: unc_model_*): 1024 (mean, stdv) pairs in k-mer order, and the one builder
// of the three tables the kernels read.  Shared by unc_host.cpp (the index's complemented tables), unc_dtw.cpp (the alignment's, not
// complemented), unc_model.cpp (the object's entry points, compiled as part of unc_host.cpp) and unc_model_acc.cpp (the training
// accumulator's finish, compiled as part of unc_align.cpp).  Host only.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <mutex>

#include "dtw_dev.h"
#include "r94_model_table.h"
#include "unc_host_util.h"

namespace unc {

// [3][1024]: lv_means_, lv_vars_x2_, lognorm_denoms_; then PoreModel::get_means_mean / get_means_stdv
struct ModelTables {
    float tab[3 * UNC_NKMER];
    float mean, stdv;
};

// PoreModel(vector, cmpl), pore_model.hpp:77-103: init_kmer (:58-62) per pair with host libm, row k ^ 0x3FF with cmpl (kmer_comp,
// bp.hpp:77-80); model_mean_ the float sum of the means in pair order over the count; init_stdv (:48-56) a float accumulator of
// double squares of float differences, in table order.  One rounding per written operation
inline void model_build_tables(const float *pairs2048, bool cmpl, ModelTables *out) {
    float *mu = out->tab, *v2 = mu + UNC_NKMER, *ld = mu + 2 * UNC_NKMER;
    float model_mean = 0;
    for (uint32_t kmer = 0; kmer < (uint32_t)UNC_NKMER; ++kmer) {
        const float mean = pairs2048[2 * kmer], stdv = pairs2048[2 * kmer + 1];
        const uint32_t k = cmpl ? kmer ^ (uint32_t)(UNC_NKMER - 1) : kmer;
        mu[k] = mean;
        float tv = 2 * stdv;
        tv = tv * stdv;
        v2[k] = tv;
        ld[k] = (float)log(sqrt(M_PI * (double)v2[k]));
        model_mean = model_mean + mean;
    }
    model_mean = model_mean / (float)UNC_NKMER;
    float acc = 0;
    for (uint32_t k = 0; k < (uint32_t)UNC_NKMER; ++k) {
        const float d = mu[k] - model_mean;
        acc = (float)((double)acc + (double)d * (double)d);
    }
    out->mean = model_mean;
    out->stdv = sqrtf(acc / (float)UNC_NKMER);
}

// the compiled-in r9.4 template pairs
inline void model_default_pairs(float *pairs2048) { memcpy(pairs2048, UNC_R94_MEAN_STDV_BITS, 2 * UNC_NKMER * sizeof(float)); }

// The exact finish of a bin of fixed-point sums (n records, S the sum of q, SS = hi * 2^64 + lo the sum of q * q, q = level * 2^20),
// shared by the training accumulator (unc_model_acc.cpp) and the pile-up (unc_pileup.cpp).  V = n * SS - S * S in unsigned 128-bit
// integers (Cauchy-Schwarz: never negative); false if n * SS leaves 128 bits
typedef unsigned __int128 u128;
inline bool sums_variance(uint64_t n, int64_t S, uint64_t lo, uint64_t hi, u128 *V) {
    const u128 SS = ((u128)hi << 64) | lo;
    if (n && SS > ~(u128)0 / n) return false;
    const u128 mag = S < 0 ? (u128)(0 - (uint64_t)S) : (u128)(uint64_t)S;
    *V = (u128)n * SS - mag * mag;
    return true;
}
// mean and deviation in levels, in double: one rounding per written operation, the 128-bit to double conversion round-to-nearest
constexpr double SUMS_Q_ONE = 1048576.0;      // 2^20, MODEL_Q_ONE of model_dev.h
inline double sums_mean(uint64_t n, int64_t S) {
    double mean = (double)S / (double)n;
    mean = mean / SUMS_Q_ONE;
    return mean;
}
inline double sums_sd(uint64_t n, u128 V) {
    double sd = sqrt((double)V);
    sd = sd / (double)n;
    sd = sd / SUMS_Q_ONE;
    return sd;
}
}  // namespace unc

// The object: immutable once made.  Its tables for the alignment (not complemented) are built with it; their copy on a device is
// uploaded by the first call that uses the model there and lives as long as the model
struct unc_model {
    float pairs[2 * UNC_NKMER];
    unc::ModelTables fwd;
    std::mutex mutex;
    DevBuf<float> dev[unc::DTW_MAX_DEVICES];
};

namespace unc {
// the model's 3 x 1024 floats (not complemented) on `device`, which is the current device: uploaded by the first call that asks
inline int model_device(const unc_model *cm, int device, const float **out) {
    unc_model *m = const_cast<unc_model *>(cm);        // (the copies on the devices are a cache: the model's value does not change)
    if (device < 0 || device >= DTW_MAX_DEVICES) return fail(UNC_ERR_ARG, "device %d", device);
    std::lock_guard<std::mutex> lk(m->mutex);
    DevBuf<float> &d = m->dev[device];
    if (!d.p) {
        DevBuf<float> buf;
        HIPCHK(buf.alloc(3 * UNC_NKMER));
        HIPCHK(hipMemcpy(buf.p, m->fwd.tab, 3 * UNC_NKMER * sizeof(float), hipMemcpyHostToDevice));
        d = std::move(buf);
    }
    *out = d.p;
    return UNC_OK;
}
}  // namespace unc
