/* uncalled_hip.h -- C ABI of libuncalled_hip.so: the MI355X (gfx950) implementation of UNCALLED's
 * per-read Mapper hot path (event detection -> normalisation -> r9.4 5-mer match -> FM-index path
 * forest -> seed clustering -> PAF coordinates), batched over reads, one wavefront per read.
 *
 * Every entry point names the reference interface it stands in for (skovaka/UNCALLED v2.3.0,
 * paths relative to the reference root).  No exceptions cross this boundary: functions return
 * UNC_OK (0) or a negative unc_status_t; unc_last_error() gives the message for the calling thread.
 * Plain pointers and sizes only -- no C++/torch types.
 */
#ifndef UNCALLED_HIP_H
#define UNCALLED_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    UNC_OK = 0,
    UNC_ERR_ARG = -1,        /* bad argument / unsupported parameter value */
    UNC_ERR_IO = -2,         /* index file missing or malformed (reference: abort(), mapper.cpp:118-127) */
    UNC_ERR_HIP = -3,        /* HIP runtime error */
    UNC_ERR_NOMEM = -4,
    UNC_ERR_OVERFLOW = -5    /* a per-read device scratch area overflowed (see unc_hit_t.status) */
} unc_status_t;

/* Compile-time shape of the kernels (the reference's defaults; mapper.cpp:30, event_detector.cpp:18-19) */
#define UNC_SEED_LEN 22
#define UNC_KLEN 5
#define UNC_NKMER 1024
#define UNC_WINDOW1 3
#define UNC_WINDOW2 6

/* Mapper::PRMS (mapper.cpp:29-52) + EventDetector::PRMS_DEF (event_detector.cpp:17-26) +
 * SeedTracker::PRMS_DEF (seed_tracker.cpp:28-32) + ReadBuffer::PRMS (read_buffer.cpp:26-32);
 * the subset Conf exposes for the map path (conf.hpp:296-340). */
typedef struct {
    uint32_t seed_len;          /* must be 22 */
    uint32_t min_rep_len;
    uint32_t max_rep_copy;      /* <= 64 */
    uint32_t max_paths;         /* <= 65535 */
    uint32_t max_consec_stay;
    uint32_t max_events;
    float max_stay_frac;
    float min_seed_prob;
    uint32_t window_length1;    /* must be 3 */
    uint32_t window_length2;    /* must be 6 */
    float threshold1, threshold2, peak_height, min_mean, max_mean;
    uint32_t min_map_len;
    float min_mean_conf, min_top_conf;
    float bp_per_sec, sample_rate;
    float chunk_time;
    uint32_t max_chunks;
} unc_params_t;

/* fast5 channel calibration, read_buffer.cpp:212-222,239-241 */
typedef struct { float range, offset, digitisation; } unc_calib_t;

/* per-read status bits */
#define UNC_READ_OK 0u
#define UNC_READ_CLUSTER_OVERFLOW 1u   /* seed-cluster scratch exhausted: result for this read is invalid */
#define UNC_READ_SEED_OVERFLOW 2u      /* per-event seed list exhausted: result for this read is invalid */
#define UNC_READ_POOL_DRY 16u          /* with CLUSTER_OVERFLOW: the shared pool of cluster nodes was empty (the read's own allowance was not used up) */
#define UNC_READ_SORT_FAULT 8u        /* internal: the runs of child keys handed to the merge were not ascending (never expected; result invalid) */
#define UNC_READ_NORM_FULL 4u          /* chunked path: >= 6000 unread events.  The reference's #SKIP branch (mapper.cpp:336-351) is OUT OF SCOPE:
                                         * unc_rt_create refuses chunk_time * sample_rate > 12000 samples, below which a chunk cannot yield 6000 events
                                         * (the detector never fires on consecutive samples) -- the bit is the belt to that pair of braces */

/* per-read notes (unc_hit_t::notes): conditions under which the reference's Mapper carries state from one read into the NEXT read
 * mapped by the same thread -- which the batch path, where every read starts from a fresh Mapper, does not reproduce (with
 * `-t N > 1` the reference's own outcome then depends on which thread gets which read).  A batch whose reads carry neither
 * note is mapped exactly as `uncalled map -t 1` maps it, whatever the order.  The chunked path (unc_rt_*) reports the same two
 * bits per read -- there a channel IS one Mapper and the carry-over is reproduced, the bits only say that it happened. */
#define UNC_NOTE_PATHS_FULL 1u         /* after some event the path buffer held max_paths paths (mapper.cpp:480,507,521,543,577,607) */
#define UNC_NOTE_FLAGS_LEFT 2u         /* sources_added_ flags were still set when the read ended (mapper.cpp:88,612-623) */

/* One PAF record's worth of coordinates (Paf, read_buffer.hpp:42-126; set by Mapper::set_ref_loc,
 * mapper.cpp:708-728) plus the work counters of SURVEY.md section 8(d). */
typedef struct {
    int32_t mapped, fwd, rid;
    uint32_t status;
    uint64_t rd_st, rd_en, rd_len;      /* PAF cols 3,4,2 */
    uint64_t rf_st, rf_en, rf_len;      /* PAF cols 8,9,7 */
    uint32_t matches;                   /* PAF col 10; col 11 = rf_en - rf_st + 1 */
    uint32_t n_events;                  /* events kept by the detector over the whole read */
    uint32_t event_i;                   /* Mapper::event_i_ at the end of map_read */
    float mean_event_len;
    uint64_t n_nbr, n_sa, n_lf;         /* get_neighbor calls, SA lookups, LF steps inside them */
    /* winning SeedCluster (seed_tracker.hpp:40-66), zero when unmapped */
    uint64_t cl_ref_st, cl_ref_en_start, cl_ref_en_end;
    uint32_t cl_evt_st, cl_evt_en, cl_total_len;
    float map_ms;                       /* batch path: time the read spent on the device, first event taken up -> result written
                                         * (device wall clock; the PAF `mt` tag, mapper.cpp:197).  Reads share wavefronts in time
                                         * slices, so this is residence, not service time.  0 on the chunked / trace paths */
    uint32_t notes;                     /* UNC_NOTE_* bits: not errors, the result is valid */
    uint32_t pad_;
} unc_hit_t;

/* stage tap: per-read result of the event/normalisation kernel */
typedef struct {
    uint32_t n_events;       /* events with mean in [min_mean, max_mean] */
    uint32_t total_events;   /* all events (EventDetector::total_events_) */
    float len_sum;           /* EventDetector::len_sum_ */
    float scale, shift;      /* Normalizer::at, normalizer.cpp:114-118 */
    uint32_t pad;
} unc_evt_info_t;

typedef struct {
    uint64_t fm_start, fm_end;
    uint32_t event_moves;
    float seed_prob;
    uint16_t kmer;
    uint8_t length, consec_stays, sa_checked, pad[3];
    float prob_sums[UNC_SEED_LEN + 1];
} unc_path_t;

typedef struct {
    uint64_t ref_st, ref_en_start, ref_en_end;
    uint32_t evt_st, evt_en, total_len, pad;
} unc_cluster_t;

typedef struct unc_index unc_index_t;
typedef struct unc_mapper unc_mapper_t;

const char *unc_last_error(void);
const char *unc_version(void);
/* PCI address ("0000:c1:00.0") of HIP device `device` as this library numbers the devices (hipDeviceGetPCIBusId): what the
 * one-process-per-GPU launchers look up under /sys/bus/pci/devices/<address>/numa_node to keep a worker's host threads on its GPU's
 * NUMA node (the reference has no counterpart: its workers are threads of one process, map_pool.cpp:31-42).  UNC_OK or an error. */
int unc_device_pci_address(int device, char *out, int cap);
/* page-locked host memory for batches handed to unc_map_batch with on_device == 0 (the copy to HBM then runs at full
 * PCIe rate and asynchronously); NULL on failure */
void *unc_host_alloc(uint64_t bytes);
void unc_host_free(void *p);

/* Conf defaults: compiled-in PRMS of the reference (SURVEY.md section 5 "Config / flags") */
void unc_params_default(unc_params_t *p);

/* ---- index: replaces Mapper::load_static (mapper.cpp:109-159) = BwaIndex::load_index
 * (bwa_index.hpp:116-135: bwt_restore_bwt / bwt_restore_sa / bns_restore + the 1024 k-mer ranges)
 * + the .uncl threshold parser (mapper.cpp:123-157) + PoreModel tables (pore_model.hpp:58-103).
 * Parses <prefix>.{bwt,sa,ann,amb,uncl} on the host and uploads BWT/Occ blocks, sampled SA, k-mer
 * ranges, thresholds and the 1024x3 model table to HBM of `device`. */
int unc_index_load(const char *bwa_prefix, const char *idx_preset, int device, unc_index_t **out);
/* the same with UNC_INDEX_* flags.  UNC_INDEX_NO_DENSE_SA: the dense suffix array (six bytes a row) is not built, SA look-ups walk to the
 * BWA-sampled rows as bwt_sa does -- for callers that only step through the BWT (unc_mask_external).  Unknown flags: UNC_ERR_ARG. */
#define UNC_INDEX_NO_DENSE_SA 1u
int unc_index_load_flags(const char *bwa_prefix, const char *idx_preset, int device, uint32_t flags, unc_index_t **out);
void unc_index_free(unc_index_t *ix);
uint64_t unc_index_size(const unc_index_t *ix);                      /* BwaIndex::size, bwa_index.hpp:180-182 */
int32_t unc_index_n_seqs(const unc_index_t *ix);
const char *unc_index_seq_name(const unc_index_t *ix, int32_t rid);  /* BwaIndex::get_ref_name, :197-199 */
uint64_t unc_index_seq_len(const unc_index_t *ix, int32_t rid);      /* BwaIndex::get_ref_len, :201-203 */
/* BwaIndex::translate_loc, bwa_index.hpp:213-220 (bns_pos2rid): returns the sequence length, 0 if none */
uint64_t unc_index_translate_loc(const unc_index_t *ix, uint64_t sa_loc, int32_t *rid, uint64_t *ref_loc);
uint64_t unc_index_device_bytes(const unc_index_t *ix);
/* host copies of the derived tables (parity taps) */
void unc_index_kmer_ranges(const unc_index_t *ix, uint64_t *out2048);       /* BwaIndex::get_kmer_range */
void unc_index_thresholds(const unc_index_t *ix, float *out64);             /* Mapper::prob_threshes_ */
void unc_index_model_tables(const unc_index_t *ix, float *means1024, float *vars_x2_1024, float *lognorm1024,
                            float *model_mean, float *model_stdv);
/* device FM primitives run over arrays (parity taps for bwa_index.hpp:158-162 and :176-178) */
int unc_fm_get_neighbor(const unc_index_t *ix, uint32_t n, const uint64_t *starts, const uint64_t *ends,
                        const uint8_t *bases, uint64_t *out_starts, uint64_t *out_ends);
int unc_fm_sa(const unc_index_t *ix, uint32_t n, const uint64_t *rows, uint64_t *out);
/* device PoreModel::match_prob over all 1024 k-mers (pore_model.hpp:163-165; mapper.cpp:443-445) */
int unc_match_probs(const unc_index_t *ix, uint32_t n, const float *levels, float *out /* n x 1024 */);

/* ---- `uncalled index` (scripts/uncalled:38-78): self-alignment of sampled reference positions, the FM walk whose
 * range-size trajectories IndexParameterizer (uncalled/index.py:53-209) turns into the .uncl thresholds.  Replaces
 * self_align(bwa_prefix, sample_dist) (src/self_align_ref.cpp:34-91): positions are sampled with the same
 * srand(0)/rand() % sample_dist draw per base, the walks run on the device.  lens (host) receives up to `cap` range
 * sizes per trajectory (row-major, n_paths x cap), full_len[i] the trajectory's true length.  Call with lens == NULL
 * to get n_paths only.  Needs <prefix>.pac next to the index files. */
int unc_self_align(const unc_index_t *ix, const char *bwa_prefix, uint32_t sample_dist, uint32_t cap, uint64_t *lens,
                   uint32_t *full_len, uint64_t max_paths, uint64_t *n_paths);

/* ---- mapper: replaces N x (Mapper::new_read + Mapper::map_read) (mapper.cpp:188-207), i.e. the
 * body of MapPool::MapperThread::run (map_pool.cpp:130-158), for a whole batch of reads. */
typedef struct {
    uint32_t n_slots;        /* reads in flight = per-read scratch slots (0 = 3 x n_waves, memory permitting) */
    uint32_t max_clusters;   /* a read's allowance of the shared node pool: max_clusters / 4 nodes (of 5 clusters; 0 = 2^20);
                              * reads that outgrow it are mapped again with a 16x larger allowance */
    uint32_t max_seed_paths; /* seed-valid paths per event (0 = 2 * max_paths, the bound) */
    uint32_t slice_events;   /* with n_slots > n_waves a wavefront parks a read after this many events and takes the
                              * next task (a new read while a slot is free, else the longest-parked read); 0 = 1024 */
    uint32_t n_waves;        /* resident wavefronts of the persistent k_map grid (0 = 16 per CU) */
    uint32_t pool_chunks;    /* the seed-cluster nodes of ALL reads in flight come from one pool, a chunk of 192 KB (768 nodes) at a
                              * time: chunks in the pool (0 = 8 per slot, 24 for references of 2^26 index rows and more, 32 from 2^31 on, at
                              * most 60 % of the free HBM); k_map stops admitting reads while the pool is nearly empty, and a read
                              * that still finds it dry is mapped again after the batch */
    uint32_t sched_parts;    /* pairs of scheduler rings (free slots, parked reads): 0 = one per XCD of the device when n_slots divides
                              * into that many shares of 64 slots or more (a slot then stays with one XCD's wavefronts, whose L2 is
                              * coherent among them: no L2 write-back / invalidate when a read is parked and resumed), else one;
                              * 1 = one pair for the whole device */
    uint32_t events_reads_per_wave;   /* k_events: reads (lanes in use) per wavefront, 1..64 (0 = 64; measured on 50 k reads:
                              * 64 -> 27 ms, 32 -> 36 ms: the kernel is bound by instruction issue) */
} unc_mapper_opts_t;

int unc_mapper_create(const unc_index_t *ix, const unc_params_t *p, const unc_mapper_opts_t *opts, unc_mapper_t **out);
void unc_mapper_free(unc_mapper_t *m);
uint64_t unc_mapper_device_bytes(const unc_mapper_t *m);

/* Map a batch.  raw = concatenated int16 samples, read i = raw[offsets[i] .. offsets[i+1]);
 * calib[i] per read.  `offsets` (n_reads + 1) and `calib` (n_reads) are ALWAYS host arrays (a few bytes per read;
 * they are validated on the host and copied).  `raw` is a host pointer when on_device == 0 (the samples are copied
 * first) and a device pointer when on_device != 0 (samples already resident in HBM).  `stream` is a
 * hipStream_t (NULL = the mapper's own stream).  hits (host, n_reads) receives one record per read. */
int unc_map_batch(unc_mapper_t *m, uint32_t n_reads, const int16_t *raw, const uint64_t *offsets,
                  const unc_calib_t *calib, int on_device, void *stream, unc_hit_t *hits);
/* The same batch in two halves (unc_map_batch = the two in a row).  _begin stages the reads and launches the kernels on `stream` (NULL:
 * the mapper's own stream) and returns at once; _end waits, maps again the few reads that need it and fills hits[0 .. n_reads).  `raw`
 * (on_device != 0: a device pointer) must stay valid until _end; `offsets` and `calib` are copied by _begin (into the mapper, before it
 * returns: the caller may reuse them at once, page-locked or not).  One batch per mapper at a time; while it is in flight
 * unc_detect_events, unc_trace_begin and unc_trace_step on the same mapper fail with UNC_ERR_ARG.  What it is for: the worker loop of MapPool::MapperThread::run (map_pool.cpp:130-158) with TWO mappers over one index -- batch
 * k + 1 is begun on the second while batch k's last long reads finish on the first, and moves into the compute units as they fall idle
 * (a persistent launch ends with a few wavefronts on a few long reads: 6 % of a 50 k-read E. coli launch). */
int unc_map_batch_begin(unc_mapper_t *m, uint32_t n_reads, const int16_t *raw, const uint64_t *offsets,
                        const unc_calib_t *calib, int on_device, void *stream);
int unc_map_batch_end(unc_mapper_t *m, unc_hit_t *hits);
/* wall-clock of the kernels of the last unc_map_batch, from HIP events on the launch stream */
int unc_mapper_last_timing(const unc_mapper_t *m, float *ms_events, float *ms_map);
/* when k_map of the mapper's last batch was submitted and when it ended, in milliseconds on ONE time axis per process (HIP events
 * against a reference event): with batches of two mappers in flight at once (unc_map_batch_begin) the launches overlap, and the time
 * the kernel holds the device per batch is the union of these windows over the number of batches, not the mean of their lengths */
int unc_mapper_last_window(const unc_mapper_t *m, double *start_ms, double *end_ms);
/* shader-clock cycles summed over the reads of the last batch, per k_map phase:
 * [0] match probs, [1] extension (loop overhead), [2] sort, [3] walk, [4] full sources, [5] SA look-ups, [6] add_seed,
 * [7] rest, [8] E1 parent loads + candidates, [9] E2 FM look-ups, [10] E3 child slots, [11] E4 child records */
int unc_mapper_last_phase_cycles(const unc_mapper_t *m, uint64_t *out12);
/* the same per READ of the last batch (n_reads = the batch's): 14 words of 64 bits per read -- the twelve counters above, the read's
 * residence in device wall-clock ticks, and where it was decided (XCC_ID | HW_ID << 8).  Diagnostics: which reads, and which part of the
 * chip, pay when a launch of the same batch runs slower than the last one (the GRCh38 levels) */
int unc_mapper_last_read_cycles(const unc_mapper_t *m, uint32_t n_reads, uint64_t *out14);
/* the counters above are collected only by batches mapped while profiling is on (off by default: the counting
 * instantiation of k_map is about 2 % slower) */
void unc_mapper_set_profile(unc_mapper_t *m, int on);
/* what unc_mapper_create settled on: [0] resident wavefronts, [1] reads in flight (slots), [2] events per time slice
 * (0: one read per wavefront until it is done), [3] chunks in the seed-cluster node pool, [4] max_clusters (a read's allowance x 4) */
void unc_mapper_geometry(const unc_mapper_t *m, uint32_t *out5);
/* diagnostics: device addresses of the mapper's large allocations: [0] slots' base, [1] bytes per slot, [2] node pool's base,
 * [3] its bytes, [4] event means, [5] results */
int unc_mapper_device_addresses(const unc_mapper_t *m, uint64_t *out6);
/* pairs of scheduler rings the mapper settled on (unc_mapper_opts_t.sched_parts); 0: no time slicing (one slot per wavefront) */
uint32_t unc_mapper_sched_parts(const unc_mapper_t *m);
/* The seed-cluster node pool is sized by need.  The reference's SeedTracker is an unbounded std::set per Mapper
 * (src/seed_tracker.hpp:97-110); here its nodes come from ONE pool per mapper.  unc_mapper_create sizes the pool by a rule of
 * thumb for the first batch; after a batch that used less than an eighth of it the library shrinks it to four times the most chunks
 * (192 KB each) that were ever out at once, never below one chunk per slot, and doubles it when a batch found it dry (unless
 * unc_mapper_opts_t.pool_chunks named a size).
 * out4: [0] chunks the pool holds now, [1] high-water mark of the last batch, [2] of all batches, [3] times it was resized. */
int unc_mapper_pool_usage(const unc_mapper_t *m, uint32_t *out4);
/* reads of the last batch that found the seed-cluster node pool dry (or used up their own allowance) and were mapped again
 * after the batch, and the wall-clock milliseconds that took (part of the batch, not of unc_mapper_last_timing) */
void unc_mapper_last_remap(const unc_mapper_t *m, uint32_t *n_reads, float *ms);
/* mean lifetime of the persistent wavefronts of the last batch's k_map launch / the launch duration (both from the
 * device wall clock): 1.0 = every wavefront worked until the end, lower = idle tail behind the longest reads */
double unc_mapper_last_wave_busy(const unc_mapper_t *m);
/* In which order the reads handed to unc_map_batch are to be understood (the reference: N worker threads with one Mapper each,
 * map_pool.cpp:31-42; the ONE piece of Mapper state that Mapper::new_read does not reset is sources_added_, mapper.cpp:88,612-623):
 *   UNC_ORDER_INDEPENDENT  every read as a fresh Mapper maps it (the default).  What `uncalled map -t N` gives for every read
 *                          whose predecessor on its thread left no flag set -- all reads without UNC_NOTE_FLAGS_LEFT neighbours
 *   UNC_ORDER_T1           `uncalled map -t 1`: one Mapper, the reads of a batch in the order given, batch after batch.  A read
 *                          whose predecessor left flags set is mapped again starting from them (and so on down the chain);
 *                          unc_mapper_last_carry_over tells how many reads of the last batch that took, in how many rounds and ms.
 * Setting the order starts a new run (the carried flags are cleared). */
#define UNC_ORDER_INDEPENDENT 0
#define UNC_ORDER_T1 1
int unc_mapper_set_read_order(unc_mapper_t *m, int order);
int unc_mapper_last_carry_over(const unc_mapper_t *m, uint32_t *reads, uint32_t *rounds, float *ms);
/* what the code object says about the k_map instantiation this mapper launches (hipFuncGetAttributes): [0] VGPRs, [1] scratch
 * bytes per lane (spills), [2] static LDS bytes per wavefront, [3] max threads per block, [4] wavefronts per CU the launch
 * bounds are set for, [5] 1 = the 32-bit-row / merged-run instantiation (references below 2^32 rows) */
int unc_mapper_kernel_info(const unc_mapper_t *m, uint32_t *out6);

/* ---- chunked (realtime) path: replaces RealtimePool + per-channel Mapper::new_read(Chunk&) / add_chunk /
 * process_chunk / map_chunk (realtime_pool.cpp:74-142,349-358; mapper.cpp:210-431) with the deterministic
 * semantics of MapPoolOrd (map_pool_ord.cpp:61-112; timeouts disabled as Conf(Mode::MAP_ORD), conf.hpp:88-91):
 * one call processes at most one chunk per channel and maps every chunk completely before returning, so a
 * caller adds the next chunk of a read only after the previous one is mapped.  Per-channel state (streaming
 * event detector, EventProfiler window, rolling Normalizer -- which survives across reads, mapper.cpp:225-226 --
 * path buffers, seed clusters) stays resident in HBM between calls. */
#define UNC_RT_FIRST 1u   /* first chunk of a read: Mapper::new_read(Chunk&) (mapper.cpp:210-217) */
#define UNC_RT_LAST 2u    /* no chunk follows: a read still unmapped afterwards is given up (request_reset, realtime_pool.cpp:115-123) */
typedef struct {
    uint32_t channel;       /* 0-based channel index (Chunk::get_channel_idx) */
    uint32_t read_number;   /* Chunk::get_number */
    uint32_t flags;         /* UNC_RT_FIRST | UNC_RT_LAST */
    uint32_t n_samples;     /* <= chunk_time * sample_rate (4000) */
    uint64_t offset;        /* first sample in `raw` */
    unc_calib_t calib;      /* the channel's calibration */
    uint32_t pad;
} unc_rt_chunk_t;
#define UNC_RT_MAPPING 0    /* chunk fully mapped, read not decided yet (Mapper::chunk_mapped) */
#define UNC_RT_MAPPED 1     /* State::SUCCESS: hit holds the PAF record */
#define UNC_RT_FAILED 2     /* State::FAILURE (max_events, max_chunks, or given up): hit holds the unmapped record */
#define UNC_RT_IGNORED 3    /* chunk of a read this channel is not mapping (already finished / never started) */
typedef struct {
    int32_t state;
    int32_t ended;          /* Paf::is_ended (set_ended, mapper.cpp:389) */
    unc_hit_t hit;
} unc_rt_result_t;
typedef struct unc_rt unc_rt_t;
int unc_rt_create(const unc_index_t *ix, const unc_params_t *p, uint32_t n_channels, unc_rt_t **out);
void unc_rt_free(unc_rt_t *rt);
uint64_t unc_rt_device_bytes(const unc_rt_t *rt);
/* raw: int16 samples (host, or device when on_device != 0); chunks/results: host arrays of n_chunks.  A call that is rejected
 * with UNC_ERR_ARG leaves the unc_rt_t and results[] exactly as they were before the call. */
int unc_rt_process_chunks(unc_rt_t *rt, uint32_t n_chunks, const unc_rt_chunk_t *chunks, const int16_t *raw, int on_device,
                          void *stream, unc_rt_result_t *results);
/* the same for chunks that already hold floats -- what the reference's Chunk keeps (src/chunk.cpp:27-66: float32 as sent by
 * MinKNOW, or int16/int32 converted WITHOUT calibration) and what Mapper::new_read(Chunk&)/add_chunk hand to the event
 * detector: `offset` indexes `signal`, the chunk's `calib` is ignored */
int unc_rt_process_chunks_f32(unc_rt_t *rt, uint32_t n_chunks, const unc_rt_chunk_t *chunks, const float *signal, int on_device,
                              void *stream, unc_rt_result_t *results);
int unc_rt_last_timing(const unc_rt_t *rt, float *ms_events, float *ms_map);
/* stage tap (parity tests): what a channel's Mapper carries between chunks below the PAF -- EventDetector counters
 * (event_detector.hpp:106-128), the EventProfiler's window and queue (event_profiler.hpp:35-48) and the rolling Normalizer
 * (normalizer.hpp:74-79) with its ring.  ring (host, 6000 floats) receives the channel's ring, slots [0, norm_n) are in use. */
typedef struct {
    uint32_t det_t, det_total_events;
    float det_len_sum;
    uint32_t norm_n, norm_wr;
    uint32_t prof_n, prof_to_mask, prof_queued;
    double norm_mean, norm_varsum;
    double prof_mean, prof_varsum;
    float prof_queue[28];               /* the queued event means, oldest first (at most 26) */
} unc_rt_tap_t;
int unc_rt_tap_channel(unc_rt_t *rt, uint32_t channel, unc_rt_tap_t *out, float *ring);

/* ---- index building (`uncalled index`; replaces the suffix sort inside bwa_idx_build, src/bwa_index.hpp:92-101)
 * Stable LSD radix sort of n (key, value) pairs of 64 bits each, ascending by the low key_bits bits of the key (1..64; the bits
 * above must be zero), on device memory: keys / vals are sorted in place, tmp_keys / tmp_vals (n words each) are scratch.
 * iota != 0: the values are taken to be 0 .. n - 1 (vals need not be initialised): vals returns the sorting permutation.
 * n < 2^32.  stream: a hipStream_t or NULL. */
int unc_sort_pairs_u64(int device, uint64_t n, uint64_t *keys, uint64_t *vals, uint64_t *tmp_keys, uint64_t *tmp_vals, int key_bits,
                       int iota, void *stream);
/* The suffix array of a text of n < 2^31 symbols (codes 0..3 in host memory) into sa[0 .. n) (host memory): the suffix sort inside
 * bwa_idx_build (src/bwa_index.hpp:92-101) as prefix doubling on the device -- the radix sort above and the steps between the sorts as
 * HIP kernels (k_sort.hip), no torch.  uncalled_amd/build_index.py writes the five BWA-format index files around it. */
int unc_build_suffix_array(int device, const uint8_t *codes, uint64_t n, int64_t *sa);

/* ---- signal-to-reference alignment: replaces DTW<float, u16, Func> (src/dtw.hpp:31-186) with the two cost functions the
 * reference ships, DTWr94p (dtw.hpp:188-210: -PoreModel::match_prob of the r9.4 TEMPLATE model, pore_model.hpp:163-165) and DTWr94d
 * (dtw.hpp:212-233: |event - model mean|), for a whole batch of alignments.  Rows are the reference k-mers, columns the event
 * means.  unc_dtw_batch: full matrix, no band: every cell is the reference's float arithmetic (dtw.hpp:51-74), so scores and paths
 * are the reference's bit for bit.  Only 2 bits per cell (the back-pointer) reach HBM; the scores live in registers.
 * unc_dtw_band_batch: the same arithmetic on the cells of a band around the diagonal (below). */
#define UNC_DTW_NONE 0u   /* DTWSubSeq::NONE: global alignment */
#define UNC_DTW_ROW 1u    /* DTWSubSeq::ROW: the events may align to a sub-range of the k-mers */
#define UNC_DTW_COL 2u    /* DTWSubSeq::COL: the k-mers may align to a sub-range of the events */
#define UNC_DTW_R94P 0u   /* dtwcost_r94p, dtw.hpp:188-190 */
#define UNC_DTW_R94D 1u   /* dtwcost_r94d, dtw.hpp:212-214 */
typedef struct {
    uint32_t subseq;      /* UNC_DTW_NONE | ROW | COL */
    uint32_t cost;        /* UNC_DTW_R94P | R94D */
    float dw, hw, vw;     /* DTWParams, dtw.hpp:10-13 */
} unc_dtw_params_t;
/* the presets of dtw.hpp:15-28 as initialisers, the cost left to the caller: unc_dtw_params_t p = UNC_DTW_EVENT_QSUB(UNC_DTW_R94P); */
#define UNC_DTW_EVENT_GLOB(cost) { UNC_DTW_NONE, (cost), 2.0f, 1.0f, 100.0f }
#define UNC_DTW_EVENT_QSUB(cost) { UNC_DTW_COL, (cost), 2.0f, 1.0f, 100.0f }
#define UNC_DTW_EVENT_RSUB(cost) { UNC_DTW_ROW, (cost), 2.0f, 1.0f, 100.0f }
#define UNC_DTW_RAW_QSUB(cost) { UNC_DTW_COL, (cost), 10.0f, 1.0f, 1000.0f }
#define UNC_DTW_RAW_RSUB(cost) { UNC_DTW_ROW, (cost), 10.0f, 1.0f, 1000.0f }
#define UNC_DTW_RAW_GLOB(cost) { UNC_DTW_NONE, (cost), 10.0f, 1.0f, 1000.0f }
/* per-alignment status */
#define UNC_DTW_OK 0u
#define UNC_DTW_TOO_LARGE 1u        /* the alignment's back-pointers alone exceed the workspace: not computed, score and path_len are 0 */
#define UNC_DTW_PATH_TRUNCATED 2u   /* path_len exceeds the room the caller gave: score and path_len are right, the first pairs are written */
#define UNC_DTW_BAND_TOO_NARROW 5u   /* band calls: the band does not hold a path to the last cell: not computed, score and path_len are 0 */
#define UNC_DTW_LEFT_BAND 6u        /* band calls: the traceback met a cell outside the band and stopped (see unc_dtw_band_batch) */
#define UNC_DTW_REF_END 7u          /* unc_dtw_adapt_batch: the end cell lies in the last row: the k-mers ran out before the events did.  The
                                       result is valid as computed; a caller who can extend the reference stretch should */
typedef struct {
    float score, mean_score;        /* DTW::score / DTW::mean_score, dtw.hpp:126-132 */
    uint64_t path_len;              /* DTW::get_path().size() */
    uint32_t status, pad;
} unc_dtw_result_t;
/* n alignments in one call: alignment a takes events[ev_off[a] .. ev_off[a+1]) as columns and kmers[km_off[a] .. km_off[a+1]) as rows
 * (all host arrays; offsets ascending).  path (host, may be NULL: scores and lengths only) receives DTW::get_path() of alignment a as
 * pairs of uint32 (event j, k-mer i), end cell first, from pair index path_off[a] on, at most path_off[a+1] - path_off[a] pairs;
 * rows + cols - 1 pairs always suffice.  workspace_bytes bounds the device memory for back-pointers (0: half of the free HBM): a batch
 * that needs more runs in several rounds with the same results; an alignment that alone needs more gets UNC_DTW_TOO_LARGE and the
 * others are computed as usual.  Empty events or k-mers, a k-mer >= 1024, 2^31 or more rows or columns, or an unknown subseq / cost:
 * UNC_ERR_ARG before anything touches the device (the reference has undefined behaviour there).  stream: a hipStream_t or NULL. */
int unc_dtw_batch(int device, uint32_t n, const float *events, const uint64_t *ev_off, const uint16_t *kmers, const uint64_t *km_off,
                  const unc_dtw_params_t *prm, uint64_t workspace_bytes, unc_dtw_result_t *res, uint32_t *path,
                  const uint64_t *path_off, void *stream);
/* unc_dtw_batch within a band of half-width `band` >= 1 around the diagonal; every other argument as unc_dtw_batch.  For an
 * alignment of R rows (k-mers) and C columns (events), with W = band:
 *   centre      c(j) = floor(j * R / C), in unsigned 64-bit arithmetic;
 *   membership  cell (i, j) is in the band iff i + W >= c(j) and i <= c(j) + W.  c is non-decreasing, so a row's cells are one
 *               interval of columns;
 *   feasibility the band always holds (0, 0); it holds (R - 1, C - 1) and a connected monotone path iff ceil(R / C) <= W + 1.  An
 *               alignment that violates this gets UNC_DTW_BAND_TOO_NARROW: not computed, score and path_len 0, the others unaffected;
 *   recurrence  the reference's (dtw.hpp:51-74): the same float additions and multiplications, the same D, H, V tie rule, the same
 *               values for predecessors outside the matrix.  A predecessor inside the matrix but outside the band reads as
 *               FLT_MAX / 2, what the reference gives cells outside the matrix in a global alignment.  Cells outside the band are
 *               neither computed nor stored: work and back-pointers are about C * (2 W + 1) cells, not R * C;
 *   traceback   the reference's (dtw.hpp:100-119) from (R - 1, C - 1).  If the next cell lies outside the band -- only non-finite
 *               scores lead there: a NaN event makes its whole column choose V, a -inf event lets D win its ties against an absent
 *               cell -- the traceback stops: status UNC_DTW_LEFT_BAND, path_len counts the pairs up to and including the last cell
 *               in the band, those pairs are written, the score is the last cell's as computed.  UNC_DTW_PATH_TRUNCATED keeps its
 *               meaning; UNC_DTW_LEFT_BAND takes precedence where both apply.
 * For finite events a banded cell's value is never below its full-matrix value (float add and multiply are monotone), hence: with
 * every cell in the band (W >= R) results equal unc_dtw_batch's; with the full matrix's path inside the band, the bits of the score
 * and the whole path equal the full matrix's.  The band is global only: band == 0, or prm->subseq != UNC_DTW_NONE, is UNC_ERR_ARG
 * before anything touches the device.  workspace_bytes, rounds and UNC_DTW_TOO_LARGE go by the banded back-pointers. */
int unc_dtw_band_batch(int device, uint32_t n, const float *events, const uint64_t *ev_off, const uint16_t *kmers, const uint64_t *km_off,
                       const unc_dtw_params_t *prm, uint32_t band, uint64_t workspace_bytes, unc_dtw_result_t *res, uint32_t *path,
                       const uint64_t *path_off, void *stream);
/* unc_dtw_batch within a band of `band` = B rows that follows the path, with an open end: for a read of which only the start on the
 * reference is known.  B is 64, 128 or 256; every other argument as unc_dtw_band_batch.  For R rows (k-mers) and C columns (events)
 * the matrix is swept by anti-diagonals d = i + j, d = 0, 1, ...:
 *   band        on anti-diagonal d the band holds the B rows [lo_d, lo_d + B), row i at column j = d - i.  lo_d is a signed 32-bit
 *               value, lo_0 = -B / 2;
 *   present     the present cells of d are those of the band inside the matrix: rows i_t = max(lo_d, 0, d - (C - 1)) to
 *               i_b = min(lo_d + B - 1, R - 1, d).  They are computed; no other cell of d is;
 *   recurrence  the reference's (dtw.hpp:51-74) as unc_dtw_batch states it: the same float additions and multiplications, the same
 *               cost, the same D <= H <= V tie rule, a global start (D of (0, 0) is 0, everything else outside the matrix FLT_MAX / 2).
 *               The predecessors of (i, j) on d are H (i, j - 1) on d - 1, V (i - 1, j) on d - 1 and D (i - 1, j - 1) on d - 2; one that
 *               is not a present cell of its anti-diagonal reads as FLT_MAX / 2;
 *   move        after d is computed, with s(i) the score of (i, d - i): lo_{d+1} = lo_d + 1 ("down") if s(i_b) < s(i_t); lo_{d+1} = lo_d
 *               ("right") if s(i_t) < s(i_b); otherwise -- equal scores, i_t == i_b, or a NaN on either side, for which neither
 *               comparison holds -- down if d is odd and right if d is even.  One exception: if lo_d + B - 1 >= R - 1, the band holds
 *               the matrix's last row already and the move is right whatever the scores are (a band led by its last row, where
 *               the path runs once the k-mers are used up, would otherwise leave the matrix before the events end);
 *   end         the sweep stops after d = R + C - 2, or at the first d that has no present cell (that d is not computed);
 *   open end    the end cell is the first smallest score among the computed cells of column C - 1, scanned by ascending row from
 *               +infinity: a cell becomes the candidate if its score compares smaller, so the lowest row wins ties.  If no score
 *               compares smaller (each is NaN or +infinity) the end cell is the computed cell of column C - 1 in the highest row.
 *               The score is the end cell's;
 *   traceback   the reference's (dtw.hpp:100-119) from the end cell to (0, 0).  If it is led to a cell that was not computed -- by
 *               non-finite scores, or through a cell all of whose predecessors were absent -- it stops: UNC_DTW_LEFT_BAND, path_len
 *               counts the pairs up to and including the last computed cell, those pairs are written.  If no cell of column C - 1 was
 *               computed the status is UNC_DTW_LEFT_BAND with score 0 and path_len 0 (for valid inputs this does not occur: the last
 *               column's row catches up with a band that stays once it holds the last row; tests/test_dtw_adapt_cpu.py sweeps it);
 *   statuses    UNC_DTW_REF_END: the end cell lies in row R - 1; everything is as with UNC_DTW_OK.  Where several apply:
 *               UNC_DTW_LEFT_BAND, then UNC_DTW_PATH_TRUNCATED (the first pair written is the end cell), then UNC_DTW_REF_END.
 * For finite events a cell's value is never below its full-matrix value, hence: if the path of the full-matrix alignment with the
 * same open end lies among the computed cells, score and path are that alignment's bit for bit.  Back-pointers take 2 bits per band
 * cell plus lo_d per anti-diagonal: about (R + C) * (B / 4 + 4) bytes, which is what workspace_bytes, the rounds and
 * UNC_DTW_TOO_LARGE go by.  band not 64, 128 or 256, or prm->subseq != UNC_DTW_NONE, is UNC_ERR_ARG before anything touches the device. */
int unc_dtw_adapt_batch(int device, uint32_t n, const float *events, const uint64_t *ev_off, const uint16_t *kmers, const uint64_t *km_off,
                        const unc_dtw_params_t *prm, uint32_t band, uint64_t workspace_bytes, unc_dtw_result_t *res, uint32_t *path,
                        const uint64_t *path_off, void *stream);
/* milliseconds the DTW kernel of the calling thread's last unc_dtw_batch / unc_dtw_band_batch / unc_dtw_adapt_batch ran (HIP events on the stream, summed
 * over its rounds), the rounds it took and the bytes of back-pointers it held at most */
int unc_dtw_last_timing(float *ms_kernel, uint32_t *rounds, uint64_t *crumb_bytes);
/* host copies of the three tables of the r9.4 template model the DTW costs read (PoreModel(vector, cmpl=false), pore_model.hpp:77-103) */
void unc_dtw_model_tables(float *means1024, float *vars_x2_1024, float *lognorm1024);
/* BwaIndex::get_kmers (bwa_index.hpp:247-255): the 5-mers of bases [st, en) of sequence rid = seq_to_kmers (bp.hpp:125-146) over the
 * packed sequence <prefix>.pac, followed for fwd == 0 by kmers_revcomp (bp.hpp:82-99).  Host only.  *n receives the count
 * (en - st - 4, or 0 below five bases); out (may be NULL to ask for the count) holds up to cap k-mers. */
int unc_ref_kmers(const unc_index_t *ix, const char *bwa_prefix, int32_t rid, uint64_t st, uint64_t en, int fwd, uint16_t *out,
                  uint64_t cap, uint64_t *n);

/* ---- read-to-reference alignment: replaces the pipeline of src/dtw_test.cpp:94-176 for a batch of queries.  A query is a read of
 * the batch, a sample range [smp_st, smp_en) of it (smp_en == 0: to the end of the read; 0, 0: the whole read, dtw_test.cpp:123-132)
 * and a run of reference k-mers.  Per query, on the device and without the event means visiting the host:
 *   EventDetector::get_events on the slice (event_detector.cpp:114-126: the detector is reset at the slice's first sample),
 *   EventProfiler::get_full_mask (event_profiler.hpp:129-151: events of stalls are dropped),
 *   the target mean and deviation of the template model's levels over the query's k-mers (dtw_test.cpp:106-116),
 *   Normalizer::set_signal / pop (normalizer.cpp:31-44,114-128),
 *   DTW of the levels (columns) against the k-mers (rows), as unc_dtw_batch.
 * Only the per-query counts return between the stages: the DTW's planner lays out the back-pointers by them. */
typedef struct {
    uint32_t read;          /* index into the batch's reads; several queries may name one read */
    uint32_t pad;
    uint64_t smp_st, smp_en;
} unc_align_query_t;
#define UNC_ALIGN_DTW_PARAMS 1u     /* opts.dtw holds the DTW's parameters (else: DTWr94d, DTWSubSeq::NONE, weights 1, 1, 1 -- dtw_test.cpp:76-78,162) */
#define UNC_ALIGN_NO_MASK 2u        /* every detected event is kept */
#define UNC_ALIGN_RAW 4u            /* create_events off (dtw_test.cpp:146-148): the calibrated samples of the slice are normalised and aligned */
#define UNC_ALIGN_TARGET_MODEL 8u   /* normalise to the model's mean and deviation over all k-mers (the line commented out at dtw_test.cpp:118) */
#define UNC_ALIGN_ADAPTIVE 16u      /* opts.band is the width B of unc_dtw_adapt_batch (64, 128 or 256): the DTW stage runs as that call */
typedef struct {
    uint32_t flags;         /* UNC_ALIGN_*; a zeroed struct is dtw_test */
    uint32_t max_events;    /* a query with more columns than this is not aligned (dtw_test.cpp:156-159 uses 50000); 0 = no limit */
    unc_dtw_params_t dtw;   /* read with UNC_ALIGN_DTW_PARAMS only */
    uint32_t band;          /* 0: the full matrix; W > 0: the DTW stage runs as unc_dtw_band_batch with this half-width (global only);
                               with UNC_ALIGN_ADAPTIVE: as unc_dtw_adapt_batch with this width */
} unc_align_opts_t;
/* per-query status: UNC_DTW_OK, UNC_DTW_TOO_LARGE, UNC_DTW_PATH_TRUNCATED (with a band also UNC_DTW_BAND_TOO_NARROW and
 * UNC_DTW_LEFT_BAND, with UNC_ALIGN_ADAPTIVE UNC_DTW_LEFT_BAND and UNC_DTW_REF_END) as unc_dtw_batch / unc_dtw_band_batch /
 * unc_dtw_adapt_batch give them, or one of */
#define UNC_ALIGN_NO_COLUMNS 3u     /* nothing left to align: the slice is too short for an event, or every event was masked.  Not aligned */
#define UNC_ALIGN_TOO_MANY 4u       /* more columns than opts.max_events.  Not aligned (counts, target, scale and shift are filled) */
typedef struct {
    unc_dtw_result_t dtw;           /* zero for a query that was not aligned */
    uint32_t n_events, n_kept;      /* events detected in the slice (samples with UNC_ALIGN_RAW) / columns left after the mask */
    float tgt_mean, tgt_stdv;       /* the Normalizer's target */
    float scale, shift;             /* Normalizer::at, normalizer.cpp:114-118 */
    uint32_t status, pad;
} unc_align_result_t;
/* raw / offsets / calib / on_device: the reads, as unc_map_batch takes them.  params: the event detector's (NULL: unc_params_default).
 * opts: NULL = zeroed.  queries (host, n_queries); query q's k-mers are kmers[km_off[q] .. km_off[q+1]) (host, ascending offsets).
 * results (host, n_queries).  levels (host, may be NULL) receives the normalised columns of query q from levels[lev_off[q]] on, at
 * most lev_off[q+1] - lev_off[q] of them (a slice of n samples has at most n / 2 + 16 events): the tap that places a mismatch at a
 * stage.  path / path_off / workspace_bytes / stream: as unc_dtw_batch.  UNC_ERR_ARG before anything touches the device for a read index
 * past the batch, a slice outside its read, smp_st > smp_en with smp_en != 0, an empty k-mer run, a k-mer >= 1024 and whatever
 * unc_dtw_batch refuses in the DTW's parameters (with opts->band > 0: what unc_dtw_band_batch refuses, a subseq other than
 * UNC_DTW_NONE among it).  UNC_ERR_OVERFLOW, for the whole batch and after device work, if a slice of n samples
 * gave more than n / 2 + 16 events: the detector's windows, which are enforced, space its peaks so that this cannot happen, and the
 * return code guards that room rather than reports on a query. */
int unc_align_batch(int device, const unc_params_t *params, const unc_align_opts_t *opts, uint32_t n_reads, const int16_t *raw,
                    const uint64_t *offsets, const unc_calib_t *calib, int on_device, uint32_t n_queries, const unc_align_query_t *queries,
                    const uint16_t *kmers, const uint64_t *km_off, uint64_t workspace_bytes, unc_align_result_t *results, float *levels,
                    const uint64_t *lev_off, uint32_t *path, const uint64_t *path_off, void *stream);
/* kernel milliseconds of the calling thread's last unc_align_batch (HIP events on the stream): [0] the slices gathered (or calibrated,
 * with UNC_ALIGN_RAW), [1] event detection, [2] mask + target + normalisation, [3] the DTW (all its rounds) */
int unc_align_last_timing(float *ms4);
/* PoreModel::get_means_mean / get_means_stdv (pore_model.hpp:48-56,82-100) of the r9.4 template model: the target of
 * UNC_ALIGN_TARGET_MODEL */
void unc_align_model_target(float *mean, float *stdv);

/* ---- the packed reference on the device: replaces BwaIndex::load_pacseq (bwa_index.hpp: bns_restore's .pac read into pacseq_, once) and
 * BwaIndex::get_kmers (bwa_index.hpp:247-255) for a batch of stretches.  unc_refseq_load reads <prefix>.pac once, keeps it on the host
 * and uploads it to the device of `ix`: the file's base bytes, followed by zeroed padding so that a kernel reading whole aligned words
 * around any stretch stays inside the allocation.  The file must be what bwa writes for the index: l_pac = unc_index_size(ix) / 2
 * bases, l_pac / 4 + 2 bytes, the last of them l_pac % 4; anything else is UNC_ERR_IO with the file's name.  The offsets of the
 * sequences in the packed text (bntann1_t::offset) are computed here, once.  The object is immutable after load: calls on it from
 * several threads at once are allowed.  It must be freed BEFORE the index it was loaded for. */
typedef struct unc_refseq unc_refseq_t;
/* BwaIndex::load_pacseq, bwa_index.hpp */
int unc_refseq_load(const unc_index_t *ix, const char *bwa_prefix, unc_refseq_t **out);
void unc_refseq_free(unc_refseq_t *rs);
uint64_t unc_refseq_device_bytes(const unc_refseq_t *rs);
/* bases [st, en) of sequence rid; fwd == 0: the minus strand (kmers_revcomp, bp.hpp:82-99) */
typedef struct { int32_t rid; uint32_t fwd; uint64_t st, en; } unc_ref_stretch_t;
/* BwaIndex::get_kmers (bwa_index.hpp:247-255) = seq_to_kmers (bp.hpp:125-146) and kmers_revcomp (bp.hpp:82-99) on the device, for n
 * stretches in one launch of k_ref_kmers: what unc_ref_kmers gives for each.  The n_a = en - st - 4 k-mers of stretch a (0 below five
 * bases: legal, nothing is written) go to out[out_off[a] .. out_off[a] + n_a); out_off (n + 1, ascending) must leave room; out is
 * host memory, and nothing outside the counts is written.  UNC_ERR_ARG before the device is touched, and with `out` untouched, for a
 * rid out of range, st > en, en past the sequence, room smaller than the count, descending offsets.  n == 0: UNC_OK. */
int unc_refseq_kmers_batch(const unc_refseq_t *rs, uint32_t n, const unc_ref_stretch_t *stretches, uint16_t *out,
                           const uint64_t *out_off, void *stream);
/* unc_align_batch with coordinates in place of k-mer arrays (dtw_test.cpp:94-105: get_kmers per query, here for the batch on the
 * device): query q's rows are the k-mers of stretches[q], made by k_ref_kmers on the stream ahead of the other stages; they reach the
 * host only when kmers_out is given (may be NULL; then query q's go to kmers_out[kmers_off[q] ..], and kmers_off, n_queries + 1 and
 * ascending, must leave room for them).  The device is the index's.  Every other argument as in unc_align_batch, and for the same
 * reads, queries and options every result, level, path and status equals, bit for bit, what unc_align_batch gives when fed
 * unc_ref_kmers' output for the same stretches.  UNC_ERR_ARG before the device is touched for what unc_align_batch refuses, for a
 * stretch that unc_refseq_kmers_batch refuses, and for a stretch of fewer than five bases (the query has no k-mers). */
int unc_align_ref_batch(const unc_refseq_t *rs, const unc_params_t *params, const unc_align_opts_t *opts, uint32_t n_reads,
                        const int16_t *raw, const uint64_t *offsets, const unc_calib_t *calib, int on_device, uint32_t n_queries,
                        const unc_align_query_t *queries, const unc_ref_stretch_t *stretches, uint64_t workspace_bytes,
                        unc_align_result_t *results, float *levels, const uint64_t *lev_off, uint16_t *kmers_out,
                        const uint64_t *kmers_off, uint32_t *path, const uint64_t *path_off, void *stream);
/* kernel milliseconds of k_ref_kmers in the calling thread's last unc_align_ref_batch (HIP events on the stream);
 * unc_align_last_timing keeps its four spans */
int unc_align_ref_last_timing(float *ms_kmers);

/* ---- alignments in sample coordinates: what a caller of the reference's dtw_test (src/dtw_test.cpp:162-176 prints DTW::get_path() and
 * stops) still has to work out by hand -- which samples of the read belong to which reference k-mer.  The path is pairs (column,
 * row); a column is an event that survived the detector's min_mean / max_mean test (event_detector.cpp:107-108) and the stall mask
 * (EventProfiler::get_full_mask, event_profiler.hpp:129-151).  The calls below keep every event's boundaries on the device and
 * collapse the path there to one record per k-mer (row) on it. */
/* Event (event_detector.hpp; create_event, event_detector.cpp:296-319): mean and stdv in pA, the event's first sample in the
 * query's slice and its samples.  With UNC_ALIGN_RAW a column is a sample: start = its index, length 1, stdv 0, mean the sample. */
typedef struct { float mean, stdv; uint32_t start, length; } unc_event_t;
/* one k-mer (row) of an alignment's path, over the row's columns c in ascending order (m, d, l: mean, stdv, length of the column's
 * event), all in double, one rounding per operation:  S += m * l;  Q += l * (d * d + m * m);  N += l;  M = S / N;
 * mean = (float)M;  stdv = (float)sqrt(fmax(Q / N - M * M, 0)) */
typedef struct {
    uint64_t smp_st;            /* first sample of the row's first event, in the READ's samples: the query's smp_st + that event's start */
    uint32_t smp_span;          /* from smp_st to the end of the row's last event; samples of events dropped in between are included */
    uint32_t smp_n;             /* sum of the lengths of the row's events (<= smp_span) */
    uint32_t col_first, n_cols; /* the row's columns on the path: [col_first, col_first + n_cols) */
    float mean, stdv;           /* pA, over the row's events, as above */
    float level;                /* Normalizer::at of mean (normalizer.cpp:114-118): scale * mean + shift, unfused, the query's scale and shift */
    uint32_t shared;            /* 1: col_first is also the previous row's last column (a vertical move: several k-mers on one event) */
} unc_segment_t;
#define UNC_SEG_OK 0u
#define UNC_SEG_TRUNCATED 1u    /* the caller's room is smaller than n_rows: the first records are written, as many as the room holds */
#define UNC_SEG_NONE 2u         /* the query's status is none of UNC_DTW_OK, UNC_DTW_PATH_TRUNCATED and UNC_DTW_REF_END: no path, no records, n_rows 0 */
/* the rows on a query's path are [row_first, row_first + n_rows) (DTW::get_path(), dtw.hpp:100-119: rows and columns fall by at
 * most one per pair); record s is row row_first + s */
typedef struct { uint32_t row_first, n_rows, status, pad; } unc_seg_info_t;
/* all host memory.  seg (may be NULL) receives query q's records from seg[seg_off[q]] on, at most seg_off[q+1] - seg_off[q] of them
 * (the query's k-mer count always suffices); info (may be NULL, n_queries) the rows and UNC_SEG_* (without seg the rows are counted
 * all the same and the status is UNC_SEG_OK: no record is missing where none was asked for); events (may be NULL), the tap:
 * query q's columns as events, in column order, from events[evt_off[q]] on, at most evt_off[q+1] - evt_off[q] (n_kept of the result
 * says how many there are).  Offsets ascend; nothing outside a query's room is written. */
typedef struct {
    unc_segment_t *seg;
    const uint64_t *seg_off;
    unc_seg_info_t *info;
    unc_event_t *events;
    const uint64_t *evt_off;
} unc_align_segments_t;
/* unc_align_batch / unc_align_ref_batch with `out` filled as well (k_align_segments runs on every round's paths while they are on the
 * device).  results, levels, path and the statuses -- UNC_DTW_PATH_TRUNCATED among them, which goes by the caller's room in path --
 * are those of the call without `out`, bit for bit; the records do not depend on the room in path.  UNC_ERR_ARG before the device
 * is touched, besides what those calls refuse: out NULL, seg without seg_off, events without evt_off, descending offsets. */
int unc_align_segments_batch(int device, const unc_params_t *params, const unc_align_opts_t *opts, uint32_t n_reads, const int16_t *raw,
                             const uint64_t *offsets, const unc_calib_t *calib, int on_device, uint32_t n_queries,
                             const unc_align_query_t *queries, const uint16_t *kmers, const uint64_t *km_off, uint64_t workspace_bytes,
                             unc_align_result_t *results, float *levels, const uint64_t *lev_off, uint32_t *path, const uint64_t *path_off,
                             const unc_align_segments_t *out, void *stream);
int unc_align_ref_segments_batch(const unc_refseq_t *rs, const unc_params_t *params, const unc_align_opts_t *opts, uint32_t n_reads,
                                 const int16_t *raw, const uint64_t *offsets, const unc_calib_t *calib, int on_device, uint32_t n_queries,
                                 const unc_align_query_t *queries, const unc_ref_stretch_t *stretches, uint64_t workspace_bytes,
                                 unc_align_result_t *results, float *levels, const uint64_t *lev_off, uint16_t *kmers_out,
                                 const uint64_t *kmers_off, uint32_t *path, const uint64_t *path_off, const unc_align_segments_t *out,
                                 void *stream);
/* kernel milliseconds of k_align_segments in the calling thread's last alignment call (HIP events on the stream, summed over the
 * DTW's rounds; 0 for a call without segments); unc_align_last_timing keeps its four spans, of which [1] is then the event
 * kernel's variant that writes whole Events (create_event, event_detector.cpp:296-319) */
int unc_align_segments_last_timing(float *ms);

/* ---- the pore model as an object: replaces PoreModel (src/pore_model.hpp) where the reference honours model_path
 * (Mapper::load_static, src/mapper.cpp:113-115).  1024 (level_mean, level_stdv) pairs in k-mer order AAAAA..TTTTT (first base most
 * significant, bp.hpp:69-75).  Immutable once made; calls on one model from several threads are allowed.  A model that an index,
 * an alignment call or an accumulator's finish was given may be freed as soon as that call has returned. */
typedef struct unc_model unc_model_t;
/* the compiled-in r9.4 template pairs: the reference's preset of src/model_r94.inl (mapper.cpp:27,57) through pore_model.hpp:77-103 */
int unc_model_default(unc_model_t **out);
/* PoreModel(vector, cmpl), pore_model.hpp:77-103: means_stdvs2048[2 k] and [2 k + 1] are k-mer k's mean and stdv.  UNC_ERR_ARG for
 * a value that is not finite or a stdv <= 0 (the reference takes anything) */
int unc_model_from_pairs(const float *means_stdvs2048, unc_model_t **out);
/* PoreModel(fname, cmpl), pore_model.hpp:108-160: one header line is skipped, then 1024 whitespace-separated `kmer mean stdv`
 * triples in any k-mer order, the k-mer read as str_to_kmer does (bp.hpp:69-75).  Departures from the reference, which prints an
 * error and returns a half-loaded model on a short file or a bad k-mer: this call fails with UNC_ERR_ARG and a message (UNC_ERR_IO
 * for a file that cannot be read) and makes no model, and it also fails on a k-mer string that is not five of ACGT, a duplicate
 * k-mer, a missing k-mer, anything behind the 1024th triple, a value that is not a finite number and stdv <= 0.  The reference
 * sums model_mean_ in the file's order (:153); here the pairs are stored by k-mer and every sum runs in k-mer order, which is the
 * file's order for a file written as the reference's uncalled/conf/r94_5mers.txt is, ascending. */
int unc_model_load(const char *path, unc_model_t **out);
/* the header line of the reference's uncalled/conf/r94_5mers.txt ("kmer\tlevel_mean\tlevel_stdv"), then the k-mers ascending as
 * "%s\t%.9g\t%.9g": nine significant digits name a float exactly, so unc_model_load of the file gives the model back in every bit */
int unc_model_save(const unc_model_t *m, const char *path);
int unc_model_pairs(const unc_model_t *m, float *out2048);
/* lv_means_, lv_vars_x2_, lognorm_denoms_ (init_kmer, pore_model.hpp:58-62), get_means_mean and get_means_stdv (init_stdv, :48-56);
 * cmpl != 0: row k ^ 0x3FF holds k-mer k (kmer_comp, bp.hpp:77-80), as the mapper's model (mapper.cpp:57) and
 * unc_index_model_tables; cmpl == 0: as dtw_test's (dtw_test.cpp:79) and unc_dtw_model_tables.  Any output may be NULL */
int unc_model_tables(const unc_model_t *m, int cmpl, float *means1024, float *vars_x2_1024, float *lognorm1024, float *model_mean,
                     float *model_stdv);
void unc_model_free(unc_model_t *m);
/* Mapper::load_static's `model = PoreModel(PRMS.model_path, true)` (mapper.cpp:113-115): the index's model tables on the host and
 * on the device become the model's, complemented.  Every later reader sees them: the normaliser's target, unc_match_probs, the
 * mapping kernels.  Allowed only while no mapper and no realtime object has EVER been made from the index (the index counts what it hands out and
 * does not count back when one is freed: load the index again for another model):
 * UNC_ERR_ARG otherwise, and nothing changes.  Waits for the device. */
int unc_index_set_model(unc_index_t *ix, const unc_model_t *m);
/* unc_dtw_batch (band == 0) / unc_dtw_band_batch (band > 0) with the costs taken from `model` (NULL: the r9.4 template, as those
 * calls).  The model's tables are uploaded to `device` once and kept with the model. */
int unc_dtw_model_batch(int device, const unc_model_t *model, uint32_t n, const float *events, const uint64_t *ev_off,
                        const uint16_t *kmers, const uint64_t *km_off, const unc_dtw_params_t *prm, uint32_t band,
                        uint64_t workspace_bytes, unc_dtw_result_t *res, uint32_t *path, const uint64_t *path_off, void *stream);

/* ---- training a model: per-k-mer statistics of the alignments' records, accumulated on the device.  The reference ships its model
 * as a file (uncalled/conf/r94_5mers.txt read by pore_model.hpp:108-160) and has no trainer; this is the counterpart that makes such
 * a file from alignments.  Per k-mer the accumulator holds n, S = sum of q and SS = sum of q * q (128 bits), with
 * q = llrint((double)level * 2^20), round to nearest even.  All integers: the sums do not depend on the order of the records, on how
 * a batch is cut into rounds, on workspace_bytes or on the caller's room in seg or path.
 * A record is DROPPED and counted (n_dropped) when its level is not finite or |level| >= 2048 (q * q then stays below 2^62).
 * A record with shared == 1 (a vertical move: several k-mers on one event) is skipped and not counted, unless the accumulator was
 * made with UNC_MODEL_KEEP_SHARED.  Queries with UNC_SEG_NONE contribute nothing.
 * One accumulator may be used by one call at a time.  A call that FAILS after device work has begun (a HIP error, an allocation
 * that fails in a later round, UNC_ERR_OVERFLOW) may have added the records of the rounds it completed: the accumulator's contents
 * are then undefined, and the caller resets it (unc_model_acc_reset) and adds again.  A call refused with UNC_ERR_ARG has added nothing. */
typedef struct unc_model_acc unc_model_acc_t;
#define UNC_MODEL_KEEP_SHARED 1u
int unc_model_acc_create(int device, uint32_t flags, unc_model_acc_t **out);
void unc_model_acc_free(unc_model_acc_t *acc);
int unc_model_acc_reset(unc_model_acc_t *acc);
/* the alignment's kernel over n records in host memory: k-mer, level and shared of record i (shared may be NULL: all 0).
 * UNC_ERR_ARG, before the device is touched, for a k-mer >= 1024.  Returns when the records are added. */
int unc_model_acc_add(unc_model_acc_t *acc, uint64_t n, const uint16_t *kmers, const float *levels, const uint32_t *shared,
                      void *stream);
/* any output may be NULL; S is the signed sum; SS = SS_hi * 2^64 + SS_lo */
int unc_model_acc_read(const unc_model_acc_t *acc, uint64_t *n1024, int64_t *S1024, uint64_t *SS_lo1024, uint64_t *SS_hi1024,
                       uint64_t *n_dropped);
/* kernel milliseconds of k_model_accum in the calling thread's last unc_model_acc_add or alignment call (HIP events on the stream,
 * summed over the DTW's rounds; 0 for a call without an accumulator) */
int unc_model_acc_last_timing(float *ms);
/* host side, exact.  For each k-mer, in unsigned 128-bit integers, V = n * SS - S * S (never negative).  If n < max(min_obs, 2) or
 * V == 0 the row is the prior's pair and is counted in n_kept_prior (may be NULL).  Otherwise
 *   mean = (float)((double)S / (double)n / 1048576.0),  stdv = (float)(sqrt((double)V) / (double)n / 1048576.0),
 * one rounding per written operation, the 128-bit to double conversion round-to-nearest.  prior NULL: the r9.4 template.
 * UNC_ERR_ARG if n * SS leaves 128 bits (more than 2^64 / 2^62 records of the largest level in one bin: not reachable). */
int unc_model_acc_finish(const unc_model_acc_t *acc, const unc_model_t *prior, uint32_t min_obs, unc_model_t **out,
                         uint32_t *n_kept_prior);

/* ---- the general alignment call: one record for everything the four entry points above take, a model and an accumulator.
 * `size` is sizeof(unc_align_call_t) as the caller was compiled: fields behind it are read as zero.  Rows come either as k-mer
 * arrays (kmers, km_off: unc_align_batch) or as coordinates (refseq, stretches, optionally kmers_out / kmers_off:
 * unc_align_ref_batch; `device` is then the reference's) -- exactly one of the two.  segs (may be NULL): the outputs of the
 * _segments_ calls.  model (may be NULL: the r9.4 template): the DTW's costs, the target over the query's k-mers and the target of
 * UNC_ALIGN_TARGET_MODEL all come from its tables, not complemented.  accumulate (may be NULL): k_model_accum runs behind
 * k_align_segments on every round, over the round's records where they lie on the device; the records need not be asked for
 * (segs NULL, or segs->seg NULL: nothing is copied to the host for it).  The accumulator must be on the call's device.
 * The four entry points above are fills of this record with model and accumulate NULL. */
typedef struct {
    uint32_t size;
    int device;
    const unc_params_t *params;
    const unc_align_opts_t *opts;
    uint32_t n_reads;
    int on_device;
    const int16_t *raw;
    const uint64_t *offsets;
    const unc_calib_t *calib;
    uint32_t n_queries;
    uint32_t pad;
    const unc_align_query_t *queries;
    const uint16_t *kmers;
    const uint64_t *km_off;
    const unc_refseq_t *refseq;
    const unc_ref_stretch_t *stretches;
    uint16_t *kmers_out;
    const uint64_t *kmers_off;
    uint64_t workspace_bytes;
    unc_align_result_t *results;
    float *levels;
    const uint64_t *lev_off;
    uint32_t *path;
    const uint64_t *path_off;
    const unc_align_segments_t *segs;
    const unc_model_t *model;
    unc_model_acc_t *accumulate;
    void *stream;
} unc_align_call_t;
int unc_align_call(const unc_align_call_t *call);

/* ---- the signal pile-up at reference coordinates: the records of the alignments (unc_segment_t), summed per reference position and
 * strand over many reads, on the device.  The reference has no counterpart; it is the step its alignments are made for (Tombo,
 * nanocompore): the signal at a position against what the model expects there, or against a second sample's.
 * A pile-up lives on the device of an unc_refseq_t and is freed before it.  It covers a list of regions (rid, st, en) -- an
 * unc_ref_stretch_t each, fwd ignored; NULL with n_regions 0: every sequence, whole -- which the create call sorts.  A BIN is a pair
 * (position p, strand): p the forward coordinate of the leftmost base of a 5-mer, st <= p < en - 4; the minus-strand bin at p holds
 * the records of minus-strand alignments whose k-mer is the reverse complement of the forward 5-mer at p.  Bins are numbered by
 * region in sorted order, then position, then strand: bin = 2 * (positions of the regions before + p - st) + (0 plus, 1 minus), 64
 * bits wide; there are 2 * sum of max(en - st - 4, 0) of them (a region of fewer than five bases is legal and holds none).
 * Each bin holds five 64-bit words, all integers: n (records), S (the signed sum of q), SS_lo and SS_hi (the 128-bit sum of q * q),
 * D (the sum of the records' smp_n: dwell in samples), q = llrint((double)level * 2^20) as in the training accumulator.  Three
 * counters beside them; a record is looked at in this order:
 *   shared == 1      skipped and not counted, unless the pile-up was made with UNC_PILEUP_KEEP_SHARED;
 *   n_dropped        its level is not finite or |level| >= 2048;
 *   n_outside        its position lies in no region;
 *   n_added          otherwise: it is in its bin.
 * The table after a set of records does not depend on their order, on how the set is split into calls or rounds, on
 * workspace_bytes or on the caller's room in seg or path.  One pile-up may be used by one call at a time.  A call that FAILS after
 * device work has begun may have added the records of the rounds it completed: the pile-up's contents are then undefined, and the
 * caller resets it and adds again.  A call refused with UNC_ERR_ARG has added nothing. */
typedef struct unc_pileup unc_pileup_t;
#define UNC_PILEUP_KEEP_SHARED 1u
/* UNC_ERR_ARG before the device is touched: a rid out of range, st > en, en past the sequence, regions that overlap, unknown flags.
 * UNC_ERR_NOMEM when the table (40 bytes a bin) cannot be allocated. */
int unc_pileup_create(const unc_refseq_t *rs, uint32_t n_regions, const unc_ref_stretch_t *regions, uint32_t flags, unc_pileup_t **out);
void unc_pileup_free(unc_pileup_t *pu);
int unc_pileup_reset(unc_pileup_t *pu);
uint64_t unc_pileup_device_bytes(const unc_pileup_t *pu);
uint64_t unc_pileup_n_bins(const unc_pileup_t *pu);
/* any output may be NULL */
int unc_pileup_counters(const unc_pileup_t *pu, uint64_t *n_dropped, uint64_t *n_outside, uint64_t *n_added);
/* k_pileup_accum over n records in host memory: record i lies at position pos[i] of sequence rid[i], strand fwd[i] != 0 plus, with
 * level[i], smp_n[i] and shared[i] (shared may be NULL: all 0).  UNC_ERR_ARG, before the device is touched, for a rid out of range;
 * a position in no region is no error (n_outside).  Returns when the records are added. */
int unc_pileup_add(unc_pileup_t *pu, uint64_t n, const int32_t *rid, const uint64_t *pos, const uint32_t *fwd, const float *level,
                   const uint32_t *smp_n, const uint32_t *shared, void *stream);
/* unc_align_call with a pile-up (NULL: exactly unc_align_call): k_pileup_accum runs behind k_align_segments (and behind
 * k_model_accum, when there is an accumulator) on every round of the DTW, over the round's records where they lie on the device;
 * they need not be asked for.  Record s of a query with stretch (rid, fwd, st, en) is row r = row_first + s: position st + r on the
 * plus strand, en - 5 - r on the minus strand (BwaIndex::get_kmers + kmers_revcomp reverse the list: row r is the reverse complement
 * of the forward k-mer that starts at en - 5 - r).  Queries with UNC_SEG_NONE contribute nothing.  Everything the call returns is bit
 * for bit what unc_align_call returns for the same record.  UNC_ERR_ARG before the device is touched, besides what unc_align_call
 * refuses: rows given as k-mer arrays (they have no coordinates), a pile-up of another unc_refseq_t or device. */
int unc_align_pileup_call(const unc_align_call_t *call, unc_pileup_t *pileup);
/* kernel milliseconds of k_pileup_accum in the calling thread's last unc_pileup_add or alignment call (HIP events on the stream,
 * summed over the DTW's rounds; 0 for a call without a pile-up) */
int unc_pileup_last_timing(float *ms);
/* the indices of the bins with n >= min_cov in a (and in b as well, unless b is NULL), ASCENDING: an ordered compaction on the device
 * in three launches (counts per workgroup, an exclusive scan, the write).  At most cap indices are written to bins_out (may be NULL
 * with cap 0); *n_out is the full count either way.  UNC_ERR_ARG for min_cov == 0 and for a b that has other regions or lies on
 * another device. */
int unc_pileup_covered(const unc_pileup_t *a, const unc_pileup_t *b, uint64_t min_cov, uint64_t *bins_out, uint64_t cap, uint64_t *n_out);
/* kernel milliseconds of the three launches of the calling thread's last unc_pileup_covered: counts, scan, write */
int unc_pileup_covered_last_timing(float *ms3);
/* the five words (n, S, SS_lo, SS_hi, D) of n listed bins, gathered on the device: out_words[5 i ..].  UNC_ERR_ARG for a bin that
 * does not exist */
int unc_pileup_gather(const unc_pileup_t *pu, uint64_t n, const uint64_t *bins, uint64_t *out_words);
/* host only, from the region table: where bin bins[i] lies.  Any output may be NULL */
int unc_pileup_bin_locate(const unc_pileup_t *pu, uint64_t n, const uint64_t *bins, int32_t *rid, uint64_t *pos, uint32_t *fwd);
/* dst += src, word by word with the 128-bit carry, and the three counters.  Both must have the same regions (UNC_ERR_ARG); src may
 * lie on another device, and is then staged through the host */
int unc_pileup_merge(unc_pileup_t *dst, const unc_pileup_t *src);
/* Statistics of listed bins, on the host, exact.  kmer: the bin's 5-mer from the packed reference, reverse-complemented for the
 * minus strand; model_mean / model_stdv: the model's pair for it (model NULL: the r9.4 template).  In unsigned 128-bit integers
 * V = n * SS - S * S; then in double, one rounding per written operation, 128-bit values converted round-to-nearest:
 *   mean = (double)S / (double)n / 1048576.0        sd = sqrt((double)V) / (double)n / 1048576.0        dwell = (double)D / (double)n
 *   z = ((mean - (double)model_mean) / (double)model_stdv) * sqrt((double)n)
 * A bin with n == 0 gives zeros.  UNC_ERR_ARG if n * SS leaves 128 bits (not reachable, as for unc_model_acc_finish). */
typedef struct {
    uint64_t n;
    double mean, sd, dwell, z;
    float model_mean, model_stdv;
    uint32_t kmer;
    uint32_t pad;
} unc_pileup_stat_t;
int unc_pileup_stats(const unc_pileup_t *pu, const unc_model_t *model, uint64_t n, const uint64_t *bins, unc_pileup_stat_t *out);
/* Welch's statistic of two pile-ups with the same regions over listed bins, mean and sd as above:
 *   se2 = sd_a * sd_a / (double)(n_a - 1) + sd_b * sd_b / (double)(n_b - 1)        t = se2 > 0 ? (mean_a - mean_b) / sqrt(se2) : 0
 * UNC_ERR_ARG for a bin with n_a < 2 or n_b < 2.  No p-values: they would need a distribution function whose bits nothing pins. */
typedef struct { uint64_t n_a, n_b; double mean_a, mean_b, sd_a, sd_b, se2, t; } unc_pileup_cmp_t;
int unc_pileup_compare(const unc_pileup_t *a, const unc_pileup_t *b, uint64_t n, const uint64_t *bins, unc_pileup_cmp_t *out);

/* ---- level histograms of a pile-up and the two-sample Kolmogorov-Smirnov distance.  A modified base often widens or splits a
 * position's level distribution while its mean barely moves; three moments cannot show that.  A pile-up can carry a second table: 64
 * buckets of uint32_t for every bin (256 bytes a bin beside the 40, and 8 for the bin's centre), attached to an EMPTY pile-up by
 * unc_pileup_hist_enable.  Histograms are meant for REGIONS: a whole bacterial genome's are gigabytes, and a table of 2^30 bins or more
 * is refused outright.  unc_pileup_create and its flags are as they were, and a pile-up without a histogram behaves bit for bit as before
 * in every entry point.
 * Width and centres: w = llrint((double)width * 2^20), 1 <= w <= 2^31, is the bucket width in the fixed point of q; a bin's centre is
 * c = llrint((double)model_mean(kmer) * 2^20), kmer the 5-mer unc_pileup_stats reports for the bin (the forward 5-mer at the bin's
 * position, reverse-complemented for the minus strand; model NULL: the r9.4 template).  The centres are written once, when the
 * histogram is attached, by a kernel that reads the packed reference on the device; the host keeps w and the model's 1024 centres.
 * Bucket rule: a record that reaches n_added lands in exactly one bucket of its bin: with t = q - c + 32 * w (signed, 64 bits) bucket
 * t < 0 ? 0 : min(t / w, 63).  Bucket 32 begins at the centre, buckets 0 and 63 take everything beyond.  Records that are shared and
 * skipped, dropped or outside touch no bucket.  For every bin the sum of its 64 buckets equals its n, as long as n < 2^32 (a bucket
 * wraps modulo 2^32).  All integers: like the table, the histograms do not depend on the records' order, the calls or the rounds.
 * unc_pileup_add and unc_align_pileup_call feed the histogram of a pile-up that has one (k_pileup_hist_accum, a launch behind every
 * k_pileup_accum over the same records, inside the span unc_pileup_last_timing reports); unc_pileup_reset zeroes it and keeps it
 * attached (with its centres); unc_pileup_device_bytes includes it; unc_pileup_merge adds it too, and refuses with UNC_ERR_ARG, both
 * pile-ups unchanged, when one side has a histogram and the other none, or when w or the 1024 centres differ.
 * unc_pileup_hist_enable: UNC_ERR_ARG, before anything on the device is allocated or written, when the pile-up holds records
 * (n_added, n_dropped or n_outside is not 0), when it has a histogram already, when width is not finite or w is out of range, or when
 * one of the model's 1024 means is not finite or has |mean| >= 2048.  UNC_ERR_NOMEM when the table does not fit; the pile-up is then
 * as it was, without a histogram. */
int unc_pileup_hist_enable(unc_pileup_t *pu, const unc_model_t *model, float width);
/* the 64 buckets of n listed bins, gathered on the device: out_counts[64 i ..]; and their centres c.  UNC_ERR_ARG for a pile-up without
 * a histogram and for a bin that does not exist */
int unc_pileup_hist_gather(const unc_pileup_t *pu, uint64_t n, const uint64_t *bins, uint32_t *out_counts);
int unc_pileup_hist_centres(const unc_pileup_t *pu, uint64_t n, const uint64_t *bins, int64_t *out_q);
/* The two-sample Kolmogorov-Smirnov distance of two pile-ups' histograms over listed bins, on the device (k_pileup_ks: a wavefront a
 * bin, a lane a bucket), exact.  With A(k), B(k) the counts of buckets 0 .. k of the bin in a and b, n_a = A(63), n_b = B(63):
 *   num = max over k of |A(k) * n_b - B(k) * n_a|   (unsigned 64-bit products; neither can overflow below)
 *   bucket = the lowest k that attains it;  sign = +1 if A(k) * n_b > B(k) * n_a there, -1 if it is less, 0 if num == 0
 * and on the host in double, one rounding per written operation:
 *   d = (double)num / ((double)n_a * (double)n_b)        ks = d * sqrt(((double)n_a * (double)n_b) / ((double)n_a + (double)n_b))
 * d is the distance of the two empirical distributions at bucket resolution, ks the statistic scaled by the effective sample size.  No
 * p-values, for unc_pileup_compare's reason.  A bin may be listed twice; a and b may be the same object (num == 0 everywhere).
 * UNC_ERR_ARG, and then out is untouched: either pile-up has no histogram; the regions, the device, w or the centres differ; a listed
 * bin does not exist; a listed bin has n_a == 0, n_b == 0 or an n >= 2^32 (n read from the pile-up's own word: a bucket may have
 * wrapped). */
typedef struct { uint64_t n_a, n_b, num; uint32_t bucket; int32_t sign; double d, ks; } unc_pileup_ks_t;   /* 48 bytes */
int unc_pileup_ks(const unc_pileup_t *a, const unc_pileup_t *b, uint64_t n, const uint64_t *bins, unc_pileup_ks_t *out);
/* kernel milliseconds of k_pileup_ks in the calling thread's last unc_pileup_ks (HIP events on the stream) */
int unc_pileup_ks_last_timing(float *ms);

/* ---- repeat masking: replaces masking/mask_internal.sh + masking/mask_kmers.py (jellyfish) and masking/mask_external.sh (bowtie,
 * bedtools, samtools), which the reference's masking/README.md recommends for references with intergenic eukaryotic DNA.
 * A reference is one byte per base: 0..3 = A C G T (either case), everything else 4 = "not a base"; a masked base becomes 4.
 * Contigs are given by n_ctg + 1 ascending offsets from 0 to n.  A window is a run of bases inside one contig without a code >= 4.
 * A k-mer's code has its first base most significant (bp.hpp).  All results are integers and exact.
 *
 * Internal masking (mask_internal.sh:46-54), k in 1..13, iters >= 1; per iteration:
 *   1. count every window of k bases, forward strand only, overlapping ones included (jellyfish count -m k without -C, :47);
 *   2. take the k-mer with the largest count (:48-49);
 *   3. turn every base covered by an occurrence of it into 4 (mask_kmers.py:8-40) -- occurrences are found in the text as it stood
 *      at the start of the iteration, overlapping ones included (`find(kmer, i + 1)`, mask_kmers.py:27).
 * Two departures from the scripts:
 *   - ties for the largest count go to the smallest k-mer code.  The script takes the last line of `jellyfish dump -L max` (:49),
 *     whose order is that of jellyfish's hash table and not reproducible;
 *   - the loop ends early, before masking, when the largest count is below 2 (the script would mask an arbitrary k-mer that occurs
 *     once).  iters_done tells how many iterations masked something.
 *
 * External masking (mask_external.sh:59-84), 2 <= min_len <= 65535 (:33), min_copy >= 1 (:38): for every window of min_len bases of the
 * target (bedtools makewindows -w min_len -s 1, full-length windows only, :61), count = the size of the window's SA interval in a
 * loaded index = its occurrences in the index's text as BWA stores it: both strands (bowtie -v 0 searches both, :67), random bases where
 * the FASTA had N.  A window is a repeat iff count > min_copy (`$4 > min_copy`, :77); every base a repeat window covers becomes 4
 * (bedtools merge / maskfasta, :78-80).  The target's codes are the masker's; the index may be of a larger reference. */
typedef struct unc_mask unc_mask_t;
/* uploads the codes (host, n < 2^32 of them: the k-mer counters are 32 bits wide) once.  UNC_ERR_ARG before the device is touched for
 * n >= 2^32, offsets that descend or do not run from 0 to n, null pointers. */
int unc_mask_create(int device, const uint8_t *codes, uint64_t n, const uint64_t *ctg_off, uint32_t n_ctg, unc_mask_t **out);
void unc_mask_free(unc_mask_t *m);
/* parity tap: step 1 of an iteration on the text as it stands; counts_out (host) receives the 4^k counters.  k outside 1..13: UNC_ERR_ARG */
int unc_mask_kmer_counts(unc_mask_t *m, uint32_t k, uint32_t *counts_out);
/* mask_internal.sh:46-54, the whole loop on the device.  kmers_out / occ_out / bases_out (host, `iters` each) receive per iteration
 * done the k-mer's code, its occurrences (mask_kmers.py:78, "masked %d occurences") and the bases newly masked; *iters_done how many.
 * The iterations are queued in batches of 32 and the host looks at the reports between batches: a loop that ends early costs at most one
 * batch of launches that return at once, however large iters is.  k outside 1..13 or iters == 0: UNC_ERR_ARG before the device is
 * touched. */
int unc_mask_internal(unc_mask_t *m, uint32_t k, uint32_t iters, uint32_t *kmers_out, uint32_t *occ_out, uint32_t *bases_out,
                      uint32_t *iters_done);
/* mask_external.sh:59-84 against `ix`, which must be on the masker's device.  counts_out (host, may be NULL): the count of the window
 * that starts at every position, 0 where there is no window; with it every look-up runs to its end, without it a look-up stops once its
 * interval holds no more than min_copy rows (intervals only shrink): the masks are the same.  *bases_masked: bases newly masked
 * (mask_external.sh:82-84 where the target held no N inside a repeat).  min_len outside 2..65535 or min_copy == 0: UNC_ERR_ARG before
 * the device is touched. */
int unc_mask_external(unc_mask_t *m, const unc_index_t *ix, uint32_t min_len, uint32_t min_copy, uint64_t *counts_out,
                      uint64_t *bases_masked);
/* the codes as they stand, n bytes to out (host) */
int unc_mask_codes(const unc_mask_t *m, uint8_t *out);
/* kernel milliseconds of the calling thread's last unc_mask_kmer_counts / _internal / _external (HIP events on the stream): counting and
 * choosing the k-mer, flagging and covering, the FM look-ups */
int unc_mask_last_timing(float *ms_count, float *ms_cover, float *ms_fm);

/* ---- measurement aid: `reps` launches that write, then `reps` that read, n_records (made odd) scattered 64-byte records with
 * one lane per record and four 16-byte accesses per lane -- k_map's access shape with an exactly known byte count, for
 * calibrating the HBM traffic counters of rocprofv3 (tools/dev/pmc_calib.py, profiles/r02_pmc_k_map.json) */
int unc_calib_traffic(int device, uint64_t n_records, int reps);
/* loaded latency of a region of device memory: `waves` (0 = 4096) single-wavefront workgroups, every lane a chain of `steps` (0 = 2000)
 * dependent 16-byte loads over [base, base + bytes); the launch's duration in milliseconds, the best of three (diagnostics) */
int unc_calib_chase(int device, const void *base, uint64_t bytes, uint32_t waves, uint32_t steps, float *ms_out);

/* ---- stage taps (parity tests) */
/* event detection + whole-read normalisation only (EventDetector::get_means, event_detector.cpp:133-145;
 * Normalizer::set_signal, normalizer.cpp:31-44).  means (host) receives the kept event means of read i
 * at means[means_offsets[i] ..]; means_offsets (host, n_reads+1) is filled by the call. */
int unc_detect_events(unc_mapper_t *m, uint32_t n_reads, const int16_t *raw, const uint64_t *offsets,
                      const unc_calib_t *calib, float *means, uint64_t means_cap, uint64_t *means_offsets,
                      unc_evt_info_t *info);
/* step-wise trace of ONE read (Mapper::map_next, mapper.cpp:433-663): begin, then step until it
 * returns 1; after each step the live path buffer and seed clusters can be read back. */
int unc_trace_begin(unc_mapper_t *m, const int16_t *raw, uint32_t n, const unc_calib_t *calib);
int unc_trace_step(unc_mapper_t *m, uint32_t n_events /* map_next calls to run */, int *done);
int unc_trace_paths(unc_mapper_t *m, unc_path_t *out, uint32_t cap, uint32_t *n_out);
int unc_trace_clusters(unc_mapper_t *m, unc_cluster_t *out, uint32_t cap, uint32_t *n_out, unc_cluster_t *max_map,
                       float *len_sum, uint32_t *n_lens);
int unc_trace_finish(unc_mapper_t *m, unc_hit_t *hit);

#ifdef __cplusplus
}
#endif
#endif
