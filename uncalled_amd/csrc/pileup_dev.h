// What unc_pileup.cpp and unc_align.cpp (host) and k_pileup.hip (kernels) share: the pile-up's table in global memory, the region
// table, the kernels' constants, their argument records and the launch wrappers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/uncalled_hip.h"
#include "align_dev.h"

namespace unc {

constexpr uint32_t PILEUP_BLOCK = 256;                  // lanes of a workgroup, of every kernel here
constexpr uint32_t PILEUP_RECS_PER_BLOCK = 1024;        // k_pileup_accum's grid rule: one workgroup for this many records (4 a lane)
constexpr uint32_t PILEUP_SCAN_CHUNK = 1024;            // bins a workgroup of the covered-bin kernels takes: 256 contiguous bins a wavefront

// The table: an array of structs, bin b's five words at tab[5 b ..]; the three counters lie behind the last bin
constexpr uint32_t PILEUP_WORDS = 5;
constexpr uint32_t PILEUP_N = 0, PILEUP_S = 1, PILEUP_LO = 2, PILEUP_HI = 3, PILEUP_D = 4;
constexpr uint32_t PILEUP_DROPPED = 0, PILEUP_OUTSIDE = 1, PILEUP_ADDED = 2, PILEUP_COUNTERS = 3;

// One region, sorted by (rid, st): positions [st, st + n) of sequence rid are the bins 2 (bin0 + p - st) + strand, strand 0 = plus.
// n = max(en - st - 4, 0): a region of fewer than five bases stays in the table and holds no bin
struct PileupRegion {
    uint64_t st, n, bin0;
    int32_t rid;
    uint32_t pad;
};

// The optional histogram beside the table: bin b's 64 buckets of 32 bits at hist[64 b ..] (an array of rows: 256 bytes a bin, two cache
// lines) and its centre at centres[b], the model's mean for the bin's k-mer in fixed point.  A record with value q goes to bucket
// t < 0 ? 0 : min(t / w, 63), t = q - centre + 32 w: bucket 32 begins at the centre, the end buckets take everything beyond
constexpr uint32_t PILEUP_HIST_BUCKETS = 64;
__host__ __device__ inline uint32_t pileup_bucket(long long q, long long centre, long long w) {
    const long long t = q - centre + 32 * w;       // |q|, |centre| < 2^31, w <= 2^31: below 2^37
    if (t < 0) return 0u;
    const unsigned long long k = (unsigned long long)t / (unsigned long long)w;
    return k < PILEUP_HIST_BUCKETS - 1 ? (uint32_t)k : PILEUP_HIST_BUCKETS - 1;
}

struct DtwJob;
struct PileupAccum {
    unsigned long long *tab;      // 5 n_bins words, then the counters
    const PileupRegion *regions;
    uint64_t n_bins;
    uint32_t n_regions;
    uint32_t flags;               // UNC_PILEUP_*
    // the caller's arrays (jobs == null): record i is (rid[i], pos[i], fwd[i], level[i], smp_n[i], shared[i]); shared may be null (all 0)
    uint64_t n;
    const int32_t *rid;
    const uint64_t *pos;
    const uint32_t *fwd;
    const float *level;
    const uint32_t *smp_n;
    const uint32_t *shared;
    // a round of the alignment (k_align_segments has run on it): everything by DtwJob::out, as in SegArgs
    const DtwJob *jobs;
    uint32_t n_jobs;
    const unc_seg_info_t *info;
    const AlignQuery *queries;
    const uint64_t *seg_off;
    const unc_segment_t *seg;
    const unc_ref_stretch_t *stretches;
};
// n_records: the arrays' n, or the sum of the round's alignments' rows (a bound on its records)
void launch_pileup_accum(const PileupAccum &a, uint64_t n_records, hipStream_t st);

// The covered bins, ascending, in three launches.  A bin is covered when its n in `a` (and in `b`, unless null) is at least min_cov.
// counts: one word per workgroup; offsets: one more than that, the last the total
inline uint64_t pileup_scan_blocks(uint64_t n_bins) { return (n_bins + PILEUP_SCAN_CHUNK - 1) / PILEUP_SCAN_CHUNK; }
void launch_pileup_count(const unsigned long long *a, const unsigned long long *b, uint64_t n_bins, uint64_t min_cov, uint32_t *counts, hipStream_t st);
void launch_pileup_scan(const uint32_t *counts, uint64_t n_blocks, uint64_t *offsets, hipStream_t st);
void launch_pileup_write(const unsigned long long *a, const unsigned long long *b, uint64_t n_bins, uint64_t min_cov, const uint64_t *offsets,
                         uint64_t *out, uint64_t cap, hipStream_t st);
// out[5 i + w] = tab[5 bins[i] + w]; the host has checked the bins
void launch_pileup_gather(const unsigned long long *tab, const uint64_t *bins, uint64_t n, unsigned long long *out, hipStream_t st);
// dst += src, bin by bin with the 128-bit carry, and the counters; both tables have n_bins bins
void launch_pileup_merge(unsigned long long *dst, const unsigned long long *src, uint64_t n_bins, hipStream_t st);

// ---- the histogram (k_pileup_hist.hip)
struct PileupHist {
    uint32_t *hist;               // 64 n_bins buckets
    const int64_t *centres;       // n_bins centres
    int64_t w;                    // the bucket width, 1 .. 2^31
};
// k_pileup_hist_accum, launched behind k_pileup_accum over the same records with the same grid: every record that k_pileup_accum adds
// to a bin (the same tests in the same order) adds 1 to one bucket of that bin.  It counts nothing
void launch_pileup_hist_accum(const PileupAccum &a, const PileupHist &h, uint64_t n_records, hipStream_t st);
// centres[2 at + strand] = ctab[k-mer of position `at` of the table], the forward 5-mer for strand 0 and its reverse complement for
// strand 1, from the packed text: base[r] is the first base of region r in the text.  n_pos = n_bins / 2
void launch_pileup_hist_centres(const uint32_t *pac, const PileupRegion *regions, const uint64_t *base, uint32_t n_regions, uint64_t n_pos,
                                const int64_t *ctab, int64_t *centres, hipStream_t st);
// out[64 i + k] = hist[64 bins[i] + k];  out[i] = centres[bins[i]];  dst[i] += src[i] over 64 n_bins buckets.  The host has checked the bins
void launch_pileup_hist_gather(const uint32_t *hist, const uint64_t *bins, uint64_t n, uint32_t *out, hipStream_t st);
void launch_pileup_centres_gather(const int64_t *centres, const uint64_t *bins, uint64_t n, int64_t *out, hipStream_t st);
void launch_pileup_hist_merge(uint32_t *dst, const uint32_t *src, uint64_t n_bins, hipStream_t st);
// what k_pileup_ks leaves of a listed bin: the two counts, the largest |A(k) n_b - B(k) n_a|, the lowest bucket that has it and the sign there
struct PileupKs {
    uint64_t n_a, n_b, num;
    uint32_t bucket;
    int32_t sign;
};
void launch_pileup_ks(const uint32_t *hist_a, const uint32_t *hist_b, const uint64_t *bins, uint64_t n, PileupKs *out, hipStream_t st);
}  // namespace unc
