// What unc_align.cpp (host) and k_align.hip (kernels) share: the record of one query and the launch wrappers.  And what unc_align.cpp
// and unc_refseq.cpp share: the record of one call (AlignCall) and where its queries' rows come from (AlignRows).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/uncalled_hip.h"

namespace unc {

struct AlignQuery {
    uint64_t src_off;             // the slice's first sample in the batch's samples
    uint64_t dst_off;             // its first sample among the gathered slices (the slices lie one after the other there)
    uint64_t col_off;             // first float of the query's room in the means and in the levels
    uint64_t km_off;              // first k-mer
    uint32_t n_smp, n_km;
    uint32_t col_cap;             // floats of room
    uint32_t pad;
    unc_calib_t calib;            // of the query's read
    uint32_t pad2;
};

struct AlignRecord {              // what the host reads back per query
    uint32_t n_events, n_kept;
    float tgt_mean, tgt_stdv, scale, shift;
    uint32_t pad[2];
};

struct AlignPrep {
    const AlignQuery *queries;
    uint32_t n_queries;
    uint32_t flags;               // UNC_ALIGN_*
    const unc_evt_info_t *info;   // k_events' counts per query (null with UNC_ALIGN_RAW: the columns are the slice's samples)
    const float *means;           // kept event means (or calibrated samples), query q from col_off on
    float *levels;                // out: the columns the DTW reads, same layout
    const uint16_t *kmers;
    const float *model;           // [3][1024] of the template model; the means are the first 1024
    float model_mean, model_stdv; // the target of UNC_ALIGN_TARGET_MODEL
    AlignRecord *rec;
    uint32_t *col_evt;            // out, may be null: col_evt[col_off + c] = the kept event that became column c (not written with UNC_ALIGN_RAW)
};

struct DtwJob;
// k_align_segments (k_segments.hip): a round's paths, collapsed to one record per row while they lie on the device
struct SegArgs {
    const DtwJob *jobs;           // the round's; path_cap is the room of the job's path on the device, rows + cols - 1
    uint32_t n_jobs;
    uint32_t raw;                 // UNC_ALIGN_RAW: column c is sample c (events and col_evt are null, means holds the calibrated samples)
    const uint32_t *path;         // the round's pairs (column, row), a job's from path_off on, end cell first
    const unc_dtw_result_t *res;  // by job.out: path_len and status as k_dtw left them
    const AlignQuery *queries;    // by job.out, as everything below
    const AlignRecord *rec;       // scale and shift
    const unc_event_t *events;    // kept events, query q from col_off on
    const float *means;
    const uint32_t *col_evt;
    const uint64_t *smp_st;       // the slice's first sample in its read
    const uint64_t *seg_off;      // n_queries + 1, from 0
    unc_segment_t *seg;
    unc_seg_info_t *info;
};
void launch_align_segments(const SegArgs &a, hipStream_t st);

// slices -> one contiguous run of samples (k_events then takes every slice as a read of its own), or with `calibrated` != null the
// calibrated samples themselves, query q from col_off on
void launch_align_gather(const int16_t *raw, const AlignQuery *queries, uint32_t n_queries, int16_t *gathered, float *calibrated, hipStream_t st);
void launch_align_prep(const AlignPrep &p, hipStream_t st);

// Where the rows of a batch's queries come from.  align_run (unc_align.cpp) is the one pipeline; its callers differ in this alone:
// unc_align_batch uploads the caller's k-mers, unc_align_ref_batch (unc_refseq.cpp) has k_ref_kmers make them from coordinates.
struct AlignRows {
    virtual ~AlignRows() = default;
    // among the checks of query q, in their order: fails with a message, or says where the query's rows lie on the device (in
    // elements from the start of the array that queue() returns) and how many they are
    virtual int rows(uint32_t q, uint64_t *at, uint32_t *n) = 0;
    // after every query's checks, the last thing before the device is touched: whatever is checked over the batch as a whole
    virtual int check() = 0;
    // on the device: allocates the array and queues on `st` whatever fills it.  The array lives as long as the object
    virtual int queue(hipStream_t st, const uint16_t **d_kmers) = 0;
};
// What the four entry points (unc_align_batch, unc_align_segments_batch, unc_align_ref_batch, unc_align_ref_segments_batch) share of
// their parameters, under the names include/uncalled_hip.h gives them.  Each fills one, once.  who: the entry point's name, for the
// messages.  segs (null: none): the outputs of the two _segments_ entry points.  model and acc: unc_align_call's (uncalled_hip.h);
// pileup and stretches: unc_align_pileup_call's
struct AlignCall {
    const char *who; int device; const unc_params_t *params; const unc_align_opts_t *opts;
    uint32_t n_reads; const int16_t *raw; const uint64_t *offsets; const unc_calib_t *calib; int on_device;
    uint32_t n_queries; const unc_align_query_t *queries; uint64_t workspace_bytes; unc_align_result_t *results;
    float *levels; const uint64_t *lev_off; uint32_t *path; const uint64_t *path_off; void *stream; const unc_align_segments_t *segs;
    const unc_model_t *model;       // null: the template model
    unc_model_acc_t *acc;           // null: no accumulator
    unc_pileup_t *pileup;           // null: no pile-up
    const unc_ref_stretch_t *stretches;     // (with a pile-up) the queries' coordinates, n_queries of them
};
int align_run(const AlignCall &c, AlignRows &rows);
}  // namespace unc
