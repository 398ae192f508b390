// Host side of repeat masking (include/uncalled_hip.h: unc_mask_*): the argument checks, the text's upload in the layout of
// mask_dev.h, the queue of kernels of one call (k_mask.hip) and the few numbers that come back.  The loop of mask_internal.sh runs
// on the device from its first iteration to its last: the host queues every iteration's kernels at once and reads the reports after
// the last one; an iteration that finds no k-mer twice raises a flag on the device at which the kernels queued behind it return.
#include <hip/hip_runtime.h>

#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "mask_dev.h"
#include "unc_host_util.h"

using namespace unc;

struct unc_mask {
    int device = 0;
    uint64_t n = 0;
    uint32_t blocks = 1;                 // of a grid-stride launch
    DevBuf<uint8_t> d_text;              // mask_dev.h: n bytes, then code 4 up to the next multiple of 64 and MASK_PAD beyond
    DevBuf<uint64_t> d_flags;            // one bit per position
    DevBuf<uint32_t> d_counts;           // 4^k, grown by need
    DevBuf<MaskIter> d_iter;
    DevBuf<MaskCtl> d_ctl;
    DevBuf<unsigned long long> d_bases;
    DevEvents ev;
};

static thread_local float g_ms_count = 0, g_ms_cover = 0, g_ms_fm = 0;

extern "C" int unc_mask_last_timing(float *ms_count, float *ms_cover, float *ms_fm) {
    if (!ms_count || !ms_cover || !ms_fm) return fail(UNC_ERR_ARG, "unc_mask_last_timing: null argument");
    *ms_count = g_ms_count; *ms_cover = g_ms_cover; *ms_fm = g_ms_fm;
    return UNC_OK;
}

extern "C" void unc_mask_free(unc_mask_t *m) { delete m; }

extern "C" int unc_mask_create(int device, const uint8_t *codes, uint64_t n, const uint64_t *ctg_off, uint32_t n_ctg, unc_mask_t **out) {
    static const char *who = "unc_mask_create";
    if (!out) return fail(UNC_ERR_ARG, "%s: null argument", who);
    *out = nullptr;
    if (!ctg_off || (n && !codes)) return fail(UNC_ERR_ARG, "%s: null argument", who);
    if (device < 0) return fail(UNC_ERR_ARG, "%s: device %d", who, device);
    if (n >= (1ull << 32)) return fail(UNC_ERR_ARG, "%s: %llu bases: the k-mer counters are 32 bits wide, 2^32 or more bases are not supported", who,
                                       (unsigned long long)n);
    if (ctg_off[0] != 0 || ctg_off[n_ctg] != n) return fail(UNC_ERR_ARG, "%s: the contig offsets must run from 0 to n", who);
    for (uint32_t i = 0; i < n_ctg; ++i)
        if (ctg_off[i + 1] < ctg_off[i]) return fail(UNC_ERR_ARG, "%s: the contig offsets must ascend", who);
    unc_mask *m = new unc_mask();
    struct Guard { unc_mask *p; ~Guard() { delete p; } } guard{m};
    m->device = device;
    m->n = n;
    const size_t n_pad = (size_t)((n + 63) / 64 * 64) + MASK_PAD;
    std::vector<uint8_t> text(n_pad, 4);
    for (uint64_t i = 0; i < n; ++i) text[i] = codes[i] < 4 ? codes[i] : 4;
    for (uint32_t i = 0; i < n_ctg; ++i)
        if (ctg_off[i] < n) text[ctg_off[i]] |= MASK_CTG_START;
    HIPCHK(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, device));
    m->blocks = 8u * (uint32_t)std::max(1, prop.multiProcessorCount);
    // UNC_MASK_BLOCKS (tests): a small grid, so that a short text takes every kernel's lanes round their grid-stride loops several times
    if (const char *e = getenv("UNC_MASK_BLOCKS")) { const long v = atol(e); if (v >= 1 && v < (long)m->blocks) m->blocks = (uint32_t)v; }
    HIPCHK(m->d_text.alloc(n_pad));
    HIPCHK(hipMemcpy(m->d_text.p, text.data(), n_pad, hipMemcpyHostToDevice));
    HIPCHK(m->d_flags.alloc((size_t)((n + 63) / 64)));
    HIPCHK(m->d_ctl.alloc(1));
    HIPCHK(m->d_bases.alloc(1));
    guard.p = nullptr;
    *out = m;
    return UNC_OK;
}

extern "C" int unc_mask_codes(const unc_mask_t *m, uint8_t *out) {
    if (!m || (m->n && !out)) return fail(UNC_ERR_ARG, "unc_mask_codes: null argument");
    if (!m->n) return UNC_OK;
    HIPCHK(hipSetDevice(m->device));
    HIPCHK(hipMemcpy(out, m->d_text.p, (size_t)m->n, hipMemcpyDeviceToHost));
    for (uint64_t i = 0; i < m->n; ++i) out[i] &= 7u;
    return UNC_OK;
}

static int check_k(const char *who, uint32_t k) {
    if (k < 1 || k > MASK_MAX_K) return fail(UNC_ERR_ARG, "%s: k = %u is not in 1..%u", who, k, MASK_MAX_K);
    return UNC_OK;
}

extern "C" int unc_mask_kmer_counts(unc_mask_t *m, uint32_t k, uint32_t *counts_out) {
    static const char *who = "unc_mask_kmer_counts";
    if (!m || !counts_out) return fail(UNC_ERR_ARG, "%s: null argument", who);
    if (int rc = check_k(who, k)) return rc;
    const size_t n_kmers = (size_t)1 << (2 * k);
    HIPCHK(hipSetDevice(m->device));
    HIPCHK(m->d_counts.reserve(std::max<size_t>(n_kmers, 4)));
    HIPCHK(m->ev.create(2));
    HIPCHK(hipMemsetAsync(m->d_counts.p, 0, n_kmers * sizeof(uint32_t), nullptr));
    HIPCHK(m->ev.record(0, nullptr));
    if (m->n) launch_kmer_count(m->d_text.p, m->n, k, m->d_counts.p, nullptr, m->blocks, nullptr);
    HIPCHK(hipGetLastError());
    HIPCHK(m->ev.record(1, nullptr));
    HIPCHK(hipMemcpy(counts_out, m->d_counts.p, n_kmers * sizeof(uint32_t), hipMemcpyDeviceToHost));
    g_ms_cover = g_ms_fm = 0;
    HIPCHK(m->ev.elapsed(0, 1, &g_ms_count));
    return UNC_OK;
}

// iterations queued at a time: the host reads the stop flag between batches, so that a loop that ends early costs at most this many
// iterations' worth of launches that return at once, however many were asked for
static constexpr uint32_t MASK_ITER_BATCH = 32;

extern "C" int unc_mask_internal(unc_mask_t *m, uint32_t k, uint32_t iters, uint32_t *kmers_out, uint32_t *occ_out, uint32_t *bases_out,
                                 uint32_t *iters_done) {
    static const char *who = "unc_mask_internal";
    if (!m || !kmers_out || !occ_out || !bases_out || !iters_done) return fail(UNC_ERR_ARG, "%s: null argument", who);
    if (int rc = check_k(who, k)) return rc;
    if (iters < 1) return fail(UNC_ERR_ARG, "%s: iters must be 1 or more", who);
    *iters_done = 0;
    g_ms_count = g_ms_cover = g_ms_fm = 0;
    if (!m->n) return UNC_OK;
    const size_t n_kmers = (size_t)1 << (2 * k);
    HIPCHK(hipSetDevice(m->device));
    HIPCHK(m->d_counts.reserve(std::max<size_t>(n_kmers, 4)));
    HIPCHK(m->d_iter.reserve(MASK_ITER_BATCH));
    HIPCHK(m->ev.create(3 * (size_t)MASK_ITER_BATCH));
    hipStream_t st = nullptr;
    HIPCHK(hipMemsetAsync(m->d_ctl.p, 0, sizeof(MaskCtl), st));
    uint32_t done = 0;
    std::vector<MaskIter> rep;
    for (uint32_t first = 0; first < iters; first += MASK_ITER_BATCH) {
        const uint32_t nb = std::min(MASK_ITER_BATCH, iters - first);
        HIPCHK(hipMemsetAsync(m->d_iter.p, 0, nb * sizeof(MaskIter), st));
        for (uint32_t i = 0; i < nb; ++i) {
            MaskIter *it = m->d_iter.p + i;
            HIPCHK(m->ev.record(3 * i, st));
            HIPCHK(hipMemsetAsync(m->d_counts.p, 0, n_kmers * sizeof(uint32_t), st));
            launch_kmer_count(m->d_text.p, m->n, k, m->d_counts.p, m->d_ctl.p, m->blocks, st);
            launch_kmer_argmax(m->d_counts.p, n_kmers, it, m->d_ctl.p, m->blocks, st);
            HIPCHK(m->ev.record(3 * i + 1, st));
            launch_mask_flag_kmer(m->d_text.p, m->n, k, it, m->d_ctl.p, m->d_flags.p, m->blocks, st);
            launch_mask_cover(m->d_text.p, m->n, k, m->d_flags.p, it, m->d_ctl.p, nullptr, m->blocks, st);
            HIPCHK(hipGetLastError());
            HIPCHK(m->ev.record(3 * i + 2, st));
        }
        HIPCHK(download(rep, m->d_iter.p, nb, st));
        HIPCHK(hipStreamSynchronize(st));
        for (uint32_t i = 0; i < nb; ++i) {
            float a = 0, b = 0;
            HIPCHK(m->ev.elapsed(3 * i, 3 * i + 1, &a));
            HIPCHK(m->ev.elapsed(3 * i + 1, 3 * i + 2, &b));
            g_ms_count += a; g_ms_cover += b;
        }
        uint32_t i = 0;
        for (; i < nb && (rep[i].best >> 32) >= 2; ++i, ++done) {
            kmers_out[done] = 0xFFFFFFFFu - (uint32_t)rep[i].best;
            occ_out[done] = rep[i].occ;
            bases_out[done] = rep[i].bases;
        }
        if (i < nb) break;          // no k-mer was left that occurs twice: the loop has ended on the device
    }
    *iters_done = done;
    return UNC_OK;
}

extern "C" int unc_mask_external(unc_mask_t *m, const unc_index_t *ix, uint32_t min_len, uint32_t min_copy, uint64_t *counts_out,
                                 uint64_t *bases_masked) {
    static const char *who = "unc_mask_external";
    if (!m || !ix || !bases_masked) return fail(UNC_ERR_ARG, "%s: null argument", who);
    if (min_len < 2 || min_len > 65535) return fail(UNC_ERR_ARG, "%s: min_len = %u is not in 2..65535", who, min_len);
    if (min_copy < 1) return fail(UNC_ERR_ARG, "%s: min_copy must be 1 or more", who);
    if (index_device(ix) != m->device) return fail(UNC_ERR_ARG, "%s: the index is on device %d, the masker on device %d", who, index_device(ix),
                                                   m->device);
    *bases_masked = 0;
    g_ms_count = g_ms_cover = g_ms_fm = 0;
    if (!m->n) return UNC_OK;
    HIPCHK(hipSetDevice(m->device));
    hipStream_t st = nullptr;
    DevBuf<uint64_t> d_tap;
    if (counts_out) HIPCHK(d_tap.alloc((size_t)m->n));
    HIPCHK(m->ev.create(3));
    HIPCHK(hipMemsetAsync(m->d_bases.p, 0, sizeof(unsigned long long), st));
    HIPCHK(m->ev.record(0, st));
    launch_fm_window_count(index_dev(ix), m->d_text.p, m->n, min_len, min_copy, m->d_flags.p, counts_out ? d_tap.p : nullptr, m->blocks, st);
    HIPCHK(hipGetLastError());
    HIPCHK(m->ev.record(1, st));
    launch_mask_cover(m->d_text.p, m->n, min_len, m->d_flags.p, nullptr, nullptr, m->d_bases.p, m->blocks, st);
    HIPCHK(hipGetLastError());
    HIPCHK(m->ev.record(2, st));
    unsigned long long bases = 0;
    HIPCHK(hipMemcpyAsync(&bases, m->d_bases.p, sizeof bases, hipMemcpyDeviceToHost, st));
    if (counts_out) HIPCHK(hipMemcpyAsync(counts_out, d_tap.p, (size_t)m->n * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    *bases_masked = bases;
    HIPCHK(m->ev.elapsed(0, 1, &g_ms_fm));
    HIPCHK(m->ev.elapsed(1, 2, &g_ms_cover));
    return UNC_OK;
}
