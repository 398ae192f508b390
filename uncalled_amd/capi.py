"""ctypes binding of the C ABI in include/uncalled_hip.h.

`load()` opens uncalled_amd/libuncalled_hip.so -- the gfx950 code object built by
`__graft_entry__.build()` -- and raises if it is missing: there is no CPU mapping path behind this
package.  (tests/ may pass an explicit library path to run the same kernel sources under the
lanesim CPU emulator; the package itself never does.)
"""
import ctypes as C
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
DEFAULT_LIB = HERE / "libuncalled_hip.so"

UNC_OK = 0
INDEX_NO_DENSE_SA = 1
UNC_ERR_OVERFLOW = -5


class Params(C.Structure):
    """unc_params_t: Mapper::PRMS + EventDetector/SeedTracker/ReadBuffer params (reference defaults)."""
    _fields_ = [("seed_len", C.c_uint32), ("min_rep_len", C.c_uint32), ("max_rep_copy", C.c_uint32),
                ("max_paths", C.c_uint32), ("max_consec_stay", C.c_uint32), ("max_events", C.c_uint32),
                ("max_stay_frac", C.c_float), ("min_seed_prob", C.c_float),
                ("window_length1", C.c_uint32), ("window_length2", C.c_uint32),
                ("threshold1", C.c_float), ("threshold2", C.c_float), ("peak_height", C.c_float),
                ("min_mean", C.c_float), ("max_mean", C.c_float),
                ("min_map_len", C.c_uint32), ("min_mean_conf", C.c_float), ("min_top_conf", C.c_float),
                ("bp_per_sec", C.c_float), ("sample_rate", C.c_float), ("chunk_time", C.c_float),
                ("max_chunks", C.c_uint32)]


class MapperOpts(C.Structure):
    _fields_ = [("n_slots", C.c_uint32), ("max_clusters", C.c_uint32), ("max_seed_paths", C.c_uint32),
                ("slice_events", C.c_uint32), ("n_waves", C.c_uint32), ("pool_chunks", C.c_uint32), ("sched_parts", C.c_uint32),
                ("events_reads_per_wave", C.c_uint32)]


CALIB = np.dtype([("range", "<f4"), ("offset", "<f4"), ("digitisation", "<f4")])
HIT = np.dtype([("mapped", "<i4"), ("fwd", "<i4"), ("rid", "<i4"), ("status", "<u4"),
                ("rd_st", "<u8"), ("rd_en", "<u8"), ("rd_len", "<u8"),
                ("rf_st", "<u8"), ("rf_en", "<u8"), ("rf_len", "<u8"),
                ("matches", "<u4"), ("n_events", "<u4"), ("event_i", "<u4"), ("mean_event_len", "<f4"),
                ("n_nbr", "<u8"), ("n_sa", "<u8"), ("n_lf", "<u8"),
                ("cl_ref_st", "<u8"), ("cl_ref_en_start", "<u8"), ("cl_ref_en_end", "<u8"),
                ("cl_evt_st", "<u4"), ("cl_evt_en", "<u4"), ("cl_total_len", "<u4"), ("map_ms", "<f4"),
                ("notes", "<u4"), ("pad_", "<u4")])
NOTE_PATHS_FULL, NOTE_FLAGS_LEFT = 1, 2      # unc_hit_t::notes (include/uncalled_hip.h)
ORDER_INDEPENDENT, ORDER_T1 = 0, 1           # unc_mapper_set_read_order
# every field of a hit but the timing one: what two runs over the same reads must agree on
RESULT_FIELDS = tuple(n for n in HIT.names if n != "map_ms")


def sort_pairs_device(keys_ptr, vals_ptr, tmp_keys_ptr, tmp_vals_ptr, n, key_bits=64, iota=False, device=0, stream=None, lib=None):
    """unc_sort_pairs_u64 on device pointers (the index builders pass torch tensors' data_ptr): stable LSD radix sort of n (key, value)
    pairs of 64 bits by the low key_bits of the key, in place; iota: the values are 0 .. n - 1, so `vals` returns the permutation."""
    L = lib or load()
    _check(L, L.unc_sort_pairs_u64(int(device), int(n), keys_ptr, vals_ptr, tmp_keys_ptr, tmp_vals_ptr, int(key_bits), 1 if iota else 0, stream))


def sort_pairs(keys, vals=None, key_bits=64, lib=None, device=0):
    """The same sort on host arrays (tests): staged in page-locked host memory, which the kernels read and write directly.
    -> (sorted keys uint64, values uint64); vals None = the sorting permutation."""
    L = lib or load()
    k = np.ascontiguousarray(keys, dtype=np.uint64)
    n = int(k.size)
    if n == 0:
        return k.copy(), np.zeros(0, np.uint64)
    buf = L.unc_host_alloc(4 * n * 8)
    if not buf:
        raise UncalledHipError("unc_host_alloc failed")
    try:
        a = np.ctypeslib.as_array(C.cast(buf, C.POINTER(C.c_uint64)), shape=(4 * n,))
        a[:n] = k
        if vals is not None:
            a[n:2 * n] = np.ascontiguousarray(vals, dtype=np.uint64)
        sort_pairs_device(buf, buf + 8 * n, buf + 16 * n, buf + 24 * n, n, key_bits, vals is None, device, None, L)
        return a[:n].copy(), a[n:2 * n].copy()
    finally:
        L.unc_host_free(buf)


def build_suffix_array(codes_u8, device=0, lib=None):
    """unc_build_suffix_array: the suffix array (int64) of a text of n < 2^31 symbols (codes 0..3), built on the device without torch."""
    L = lib or load()
    t = np.ascontiguousarray(codes_u8, dtype=np.uint8)
    sa = np.empty(t.size, dtype=np.int64)
    _check(L, L.unc_build_suffix_array(int(device), t.ctypes.data, int(t.size), sa.ctypes.data))
    return sa


def hits_digest(hits):
    """sha256 over the result fields of a hit array (map_ms, a wall-clock measurement, zeroed)."""
    import hashlib
    h = hits.copy()
    h["map_ms"] = 0
    return hashlib.sha256(h.tobytes()).hexdigest()


EVT_INFO = np.dtype([("n_events", "<u4"), ("total_events", "<u4"), ("len_sum", "<f4"), ("scale", "<f4"),
                     ("shift", "<f4"), ("pad", "<u4")])
PATH = np.dtype([("fm_start", "<u8"), ("fm_end", "<u8"), ("event_moves", "<u4"), ("seed_prob", "<f4"),
                 ("kmer", "<u2"), ("length", "u1"), ("consec_stays", "u1"), ("sa_checked", "u1"),
                 ("pad", "u1", 3), ("prob_sums", "<f4", 23)], align=True)
CLUSTER = np.dtype([("ref_st", "<u8"), ("ref_en_start", "<u8"), ("ref_en_end", "<u8"),
                    ("evt_st", "<u4"), ("evt_en", "<u4"), ("total_len", "<u4"), ("pad", "<u4")])

RT_CHUNK = np.dtype([("channel", "<u4"), ("read_number", "<u4"), ("flags", "<u4"), ("n_samples", "<u4"), ("offset", "<u8"),
                     ("calib", CALIB), ("pad", "<u4")])
RT_RESULT = np.dtype([("state", "<i4"), ("ended", "<i4"), ("hit", HIT)])
RT_FIRST, RT_LAST = 1, 2
RT_MAPPING, RT_MAPPED, RT_FAILED, RT_IGNORED = 0, 1, 2, 3



class DTWParams(C.Structure):
    """unc_dtw_params_t: DTWParams of the reference (dtw.hpp:10-13) plus the cost function (DTWr94p / DTWr94d)."""
    _fields_ = [("subseq", C.c_uint32), ("cost", C.c_uint32), ("dw", C.c_float), ("hw", C.c_float), ("vw", C.c_float)]

    def with_cost(self, cost):
        return DTWParams(self.subseq, cost, self.dw, self.hw, self.vw)


DTW_NONE, DTW_ROW, DTW_COL = 0, 1, 2                  # DTWSubSeq
DTW_R94P, DTW_R94D = 0, 1                             # dtwcost_r94p / dtwcost_r94d
DTW_OK, DTW_TOO_LARGE, DTW_PATH_TRUNCATED = 0, 1, 2   # unc_dtw_result_t.status
DTW_BAND_TOO_NARROW, DTW_LEFT_BAND = 5, 6             # ... of band calls (3 and 4 are the ALIGN_* ones below)
DTW_REF_END = 7                                       # ... of adaptive calls: the end cell lies in the last row, the result is valid
# the presets of dtw.hpp:15-28 (cost r94p; .with_cost(DTW_R94D) for the other)
DTW_EVENT_GLOB = DTWParams(DTW_NONE, DTW_R94P, 2, 1, 100)
DTW_EVENT_QSUB = DTWParams(DTW_COL, DTW_R94P, 2, 1, 100)
DTW_EVENT_RSUB = DTWParams(DTW_ROW, DTW_R94P, 2, 1, 100)
DTW_RAW_QSUB = DTWParams(DTW_COL, DTW_R94P, 10, 1, 1000)
DTW_RAW_RSUB = DTWParams(DTW_ROW, DTW_R94P, 10, 1, 1000)
DTW_RAW_GLOB = DTWParams(DTW_NONE, DTW_R94P, 10, 1, 1000)
DTW_RESULT = np.dtype([("score", "<f4"), ("mean_score", "<f4"), ("path_len", "<u8"), ("status", "<u4"), ("pad", "<u4")])


class AlignOpts(C.Structure):
    """unc_align_opts_t; AlignOpts() is dtw_test: events, stall mask, target from the k-mers, DTWr94d / NONE / 1, 1, 1."""
    _fields_ = [("flags", C.c_uint32), ("max_events", C.c_uint32), ("dtw", DTWParams), ("band", C.c_uint32)]


ALIGN_DTW_PARAMS, ALIGN_NO_MASK, ALIGN_RAW, ALIGN_TARGET_MODEL = 1, 2, 4, 8       # unc_align_opts_t.flags
ALIGN_ADAPTIVE = 16                                                               # ... band is unc_dtw_adapt_batch's width
ALIGN_NO_COLUMNS, ALIGN_TOO_MANY = 3, 4                                           # unc_align_result_t.status beside the DTW_* ones
ALIGN_QUERY = np.dtype([("read", "<u4"), ("pad", "<u4"), ("smp_st", "<u8"), ("smp_en", "<u8")])
ALIGN_RESULT = np.dtype([("dtw", DTW_RESULT), ("n_events", "<u4"), ("n_kept", "<u4"), ("tgt_mean", "<f4"), ("tgt_stdv", "<f4"),
                         ("scale", "<f4"), ("shift", "<f4"), ("status", "<u4"), ("pad", "<u4")])

# unc_event_t (the reference's Event), unc_segment_t, unc_seg_info_t
EVENT = np.dtype([("mean", "<f4"), ("stdv", "<f4"), ("start", "<u4"), ("length", "<u4")])
SEGMENT = np.dtype([("smp_st", "<u8"), ("smp_span", "<u4"), ("smp_n", "<u4"), ("col_first", "<u4"), ("n_cols", "<u4"), ("mean", "<f4"),
                    ("stdv", "<f4"), ("level", "<f4"), ("shared", "<u4")])
SEG_INFO = np.dtype([("row_first", "<u4"), ("n_rows", "<u4"), ("status", "<u4"), ("pad", "<u4")])
SEG_OK, SEG_TRUNCATED, SEG_NONE = 0, 1, 2


class AlignSegments(C.Structure):
    """unc_align_segments_t: where the records, the rows' counts and the tapped events go (host addresses; 0 = not wanted)"""
    _fields_ = [("seg", C.c_void_p), ("seg_off", C.c_void_p), ("info", C.c_void_p), ("events", C.c_void_p), ("evt_off", C.c_void_p)]


REF_STRETCH = np.dtype([("rid", "<i4"), ("fwd", "<u4"), ("st", "<u8"), ("en", "<u8")])      # unc_ref_stretch_t
MODEL_KEEP_SHARED = 1
PILEUP_KEEP_SHARED = 1
# unc_pileup_stat_t, unc_pileup_cmp_t; a bin's five words as unc_pileup_gather returns them
PILEUP_STAT = np.dtype([("n", "<u8"), ("mean", "<f8"), ("sd", "<f8"), ("dwell", "<f8"), ("z", "<f8"), ("model_mean", "<f4"), ("model_stdv", "<f4"),
                        ("kmer", "<u4"), ("pad", "<u4")])
PILEUP_CMP = np.dtype([("n_a", "<u8"), ("n_b", "<u8"), ("mean_a", "<f8"), ("mean_b", "<f8"), ("sd_a", "<f8"), ("sd_b", "<f8"), ("se2", "<f8"),
                       ("t", "<f8")])
PILEUP_WORDS = np.dtype([("n", "<u8"), ("S", "<i8"), ("SS_lo", "<u8"), ("SS_hi", "<u8"), ("D", "<u8")])
# unc_pileup_ks_t; the buckets of a bin's histogram
PILEUP_KS = np.dtype([("n_a", "<u8"), ("n_b", "<u8"), ("num", "<u8"), ("bucket", "<u4"), ("sign", "<i4"), ("d", "<f8"), ("ks", "<f8")])
PILEUP_HIST_BUCKETS = 64


class AlignCall(C.Structure):
    """unc_align_call_t: the general alignment call's record"""
    _fields_ = [("size", C.c_uint32), ("device", C.c_int), ("params", C.c_void_p), ("opts", C.c_void_p), ("n_reads", C.c_uint32),
                ("on_device", C.c_int), ("raw", C.c_void_p), ("offsets", C.c_void_p), ("calib", C.c_void_p), ("n_queries", C.c_uint32),
                ("pad", C.c_uint32), ("queries", C.c_void_p), ("kmers", C.c_void_p), ("km_off", C.c_void_p), ("refseq", C.c_void_p),
                ("stretches", C.c_void_p), ("kmers_out", C.c_void_p), ("kmers_off", C.c_void_p), ("workspace_bytes", C.c_uint64),
                ("results", C.c_void_p), ("levels", C.c_void_p), ("lev_off", C.c_void_p), ("path", C.c_void_p), ("path_off", C.c_void_p),
                ("segs", C.c_void_p), ("model", C.c_void_p), ("accumulate", C.c_void_p), ("stream", C.c_void_p)]


_libs = {}


class UncalledHipError(RuntimeError):
    pass


def load(path=None):
    """Open the shared library (default: the in-tree gfx950 build) and declare its prototypes."""
    path = Path(path) if path else DEFAULT_LIB
    key = str(path)
    if key in _libs:
        return _libs[key]
    if not path.exists():
        raise UncalledHipError(
            f"{path} not found: build the HIP extension first (python -c 'import __graft_entry__ as g; g.build()'). "
            "uncalled_amd has no CPU fallback.")
    L = C.CDLL(str(path.resolve()))
    vp, u32, u64, i32 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int32
    L.unc_last_error.restype = C.c_char_p
    L.unc_version.restype = C.c_char_p
    L.unc_calib_traffic.argtypes = [C.c_int, u64, C.c_int]
    L.unc_host_alloc.argtypes = [u64]; L.unc_host_alloc.restype = vp
    L.unc_host_free.argtypes = [vp]; L.unc_host_free.restype = None
    L.unc_params_default.argtypes = [C.POINTER(Params)]
    L.unc_index_load.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.POINTER(vp)]
    if hasattr(L, "unc_index_load_flags"):
        L.unc_index_load_flags.argtypes = [C.c_char_p, C.c_char_p, C.c_int, u32, C.POINTER(vp)]
    L.unc_index_free.argtypes = [vp]
    L.unc_index_size.argtypes = [vp]; L.unc_index_size.restype = u64
    L.unc_index_n_seqs.argtypes = [vp]; L.unc_index_n_seqs.restype = i32
    L.unc_index_seq_name.argtypes = [vp, i32]; L.unc_index_seq_name.restype = C.c_char_p
    L.unc_index_seq_len.argtypes = [vp, i32]; L.unc_index_seq_len.restype = u64
    L.unc_index_translate_loc.argtypes = [vp, u64, C.POINTER(i32), C.POINTER(u64)]; L.unc_index_translate_loc.restype = u64
    L.unc_index_device_bytes.argtypes = [vp]; L.unc_index_device_bytes.restype = u64
    L.unc_index_kmer_ranges.argtypes = [vp, vp]
    L.unc_index_thresholds.argtypes = [vp, vp]
    L.unc_index_model_tables.argtypes = [vp, vp, vp, vp, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    L.unc_fm_get_neighbor.argtypes = [vp, u32, vp, vp, vp, vp, vp]
    L.unc_fm_sa.argtypes = [vp, u32, vp, vp]
    L.unc_match_probs.argtypes = [vp, u32, vp, vp]
    L.unc_self_align.argtypes = [vp, C.c_char_p, u32, u32, vp, vp, u64, C.POINTER(u64)]
    L.unc_mapper_create.argtypes = [vp, C.POINTER(Params), C.POINTER(MapperOpts), C.POINTER(vp)]
    L.unc_mapper_free.argtypes = [vp]
    L.unc_mapper_device_bytes.argtypes = [vp]; L.unc_mapper_device_bytes.restype = u64
    L.unc_map_batch.argtypes = [vp, u32, vp, vp, vp, C.c_int, vp, vp]
    if hasattr(L, "unc_build_suffix_array"):
        L.unc_build_suffix_array.argtypes = [C.c_int, vp, u64, vp]
    if hasattr(L, "unc_mapper_last_window"):
        L.unc_mapper_last_window.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    if hasattr(L, "unc_map_batch_begin"):
        L.unc_map_batch_begin.argtypes = [vp, u32, vp, vp, vp, C.c_int, vp]
        L.unc_map_batch_end.argtypes = [vp, vp]
    L.unc_mapper_last_timing.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    L.unc_mapper_last_phase_cycles.argtypes = [vp, vp]
    L.unc_mapper_last_read_cycles.argtypes = [vp, u32, vp]
    L.unc_mapper_last_remap.argtypes = [vp, C.POINTER(u32), C.POINTER(C.c_float)]
    L.unc_mapper_last_remap.restype = None
    if hasattr(L, "unc_mapper_set_read_order"):      # (dev tools load older builds of the library for A/B runs)
        L.unc_mapper_set_read_order.argtypes = [vp, C.c_int]
        L.unc_mapper_last_carry_over.argtypes = [vp, C.POINTER(u32), C.POINTER(u32), C.POINTER(C.c_float)]
    L.unc_mapper_kernel_info.argtypes = [vp, vp]
    L.unc_mapper_kernel_info.restype = i32
    L.unc_mapper_geometry.argtypes = [vp, vp]
    L.unc_mapper_geometry.restype = None
    if hasattr(L, "unc_sort_pairs_u64"):
        L.unc_sort_pairs_u64.argtypes = [i32, u64, vp, vp, vp, vp, i32, i32, vp]
        L.unc_sort_pairs_u64.restype = C.c_int
    if hasattr(L, "unc_mapper_pool_usage"):           # (older builds under uncalled_amd/variants/ lack it)
        L.unc_mapper_pool_usage.argtypes = [vp, vp]
        L.unc_mapper_pool_usage.restype = C.c_int
    L.unc_mapper_set_profile.argtypes = [vp, C.c_int]
    L.unc_mapper_set_profile.restype = None
    L.unc_mapper_last_wave_busy.argtypes = [vp]
    L.unc_mapper_last_wave_busy.restype = C.c_double
    L.unc_detect_events.argtypes = [vp, u32, vp, vp, vp, vp, u64, vp, vp]
    L.unc_rt_create.argtypes = [vp, C.POINTER(Params), u32, C.POINTER(vp)]
    L.unc_rt_free.argtypes = [vp]
    L.unc_rt_device_bytes.argtypes = [vp]; L.unc_rt_device_bytes.restype = u64
    L.unc_rt_process_chunks.argtypes = [vp, u32, vp, vp, C.c_int, vp, vp]
    L.unc_rt_process_chunks_f32.argtypes = [vp, u32, vp, vp, C.c_int, vp, vp]
    L.unc_rt_last_timing.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    if hasattr(L, "unc_rt_tap_channel"):
        L.unc_rt_tap_channel.argtypes = [vp, u32, vp, vp]
    L.unc_trace_begin.argtypes = [vp, vp, u32, vp]
    L.unc_trace_step.argtypes = [vp, u32, C.POINTER(C.c_int)]
    L.unc_trace_paths.argtypes = [vp, vp, u32, C.POINTER(u32)]
    L.unc_trace_clusters.argtypes = [vp, vp, u32, C.POINTER(u32), vp, C.POINTER(C.c_float), C.POINTER(u32)]
    L.unc_trace_finish.argtypes = [vp, vp]
    if hasattr(L, "unc_dtw_batch"):                   # (the emulator build of the mapper's sources does not hold the DTW entry points)
        L.unc_dtw_batch.argtypes = [C.c_int, u32, vp, vp, vp, vp, C.POINTER(DTWParams), u64, vp, vp, vp, vp]
        if hasattr(L, "unc_dtw_band_batch"):
            L.unc_dtw_band_batch.argtypes = [C.c_int, u32, vp, vp, vp, vp, C.POINTER(DTWParams), u32, u64, vp, vp, vp, vp]
        if hasattr(L, "unc_dtw_adapt_batch"):
            L.unc_dtw_adapt_batch.argtypes = [C.c_int, u32, vp, vp, vp, vp, C.POINTER(DTWParams), u32, u64, vp, vp, vp, vp]
        L.unc_dtw_last_timing.argtypes = [C.POINTER(C.c_float), C.POINTER(u32), C.POINTER(u64)]
        L.unc_dtw_model_tables.argtypes = [vp, vp, vp]
        L.unc_dtw_model_tables.restype = None
        L.unc_ref_kmers.argtypes = [vp, C.c_char_p, i32, u64, u64, C.c_int, vp, u64, C.POINTER(u64)]
    if hasattr(L, "unc_align_batch"):
        L.unc_align_batch.argtypes = [C.c_int, C.POINTER(Params), C.POINTER(AlignOpts), u32, vp, vp, vp, C.c_int, u32, vp, vp, vp, u64, vp,
                                      vp, vp, vp, vp, vp]
        L.unc_align_last_timing.argtypes = [vp]
        L.unc_align_model_target.argtypes = [C.POINTER(C.c_float), C.POINTER(C.c_float)]
        L.unc_align_model_target.restype = None
    if hasattr(L, "unc_align_segments_batch"):
        L.unc_align_segments_batch.argtypes = L.unc_align_batch.argtypes[:-1] + [C.POINTER(AlignSegments), vp]
        L.unc_align_segments_last_timing.argtypes = [C.POINTER(C.c_float)]
    if hasattr(L, "unc_refseq_load"):
        L.unc_refseq_load.argtypes = [vp, C.c_char_p, C.POINTER(vp)]
        L.unc_refseq_free.argtypes = [vp]; L.unc_refseq_free.restype = None
        L.unc_refseq_device_bytes.argtypes = [vp]; L.unc_refseq_device_bytes.restype = u64
        L.unc_refseq_kmers_batch.argtypes = [vp, u32, vp, vp, vp, vp]
        L.unc_align_ref_batch.argtypes = [vp, C.POINTER(Params), C.POINTER(AlignOpts), u32, vp, vp, vp, C.c_int, u32, vp, vp, u64, vp,
                                          vp, vp, vp, vp, vp, vp, vp]
        L.unc_align_ref_last_timing.argtypes = [C.POINTER(C.c_float)]
        if hasattr(L, "unc_align_ref_segments_batch"):
            L.unc_align_ref_segments_batch.argtypes = L.unc_align_ref_batch.argtypes[:-1] + [C.POINTER(AlignSegments), vp]
    if hasattr(L, "unc_model_default"):
        L.unc_model_default.argtypes = [C.POINTER(vp)]
        L.unc_model_from_pairs.argtypes = [vp, C.POINTER(vp)]
        L.unc_model_load.argtypes = [C.c_char_p, C.POINTER(vp)]
        L.unc_model_save.argtypes = [vp, C.c_char_p]
        L.unc_model_pairs.argtypes = [vp, vp]
        L.unc_model_tables.argtypes = [vp, C.c_int, vp, vp, vp, C.POINTER(C.c_float), C.POINTER(C.c_float)]
        L.unc_model_free.argtypes = [vp]; L.unc_model_free.restype = None
        L.unc_index_set_model.argtypes = [vp, vp]
    if hasattr(L, "unc_dtw_model_batch"):
        L.unc_dtw_model_batch.argtypes = [C.c_int, vp, u32, vp, vp, vp, vp, C.POINTER(DTWParams), u32, u64, vp, vp, vp, vp]
    if hasattr(L, "unc_model_acc_create"):            # (with the alignment sources)
        L.unc_model_acc_create.argtypes = [C.c_int, u32, C.POINTER(vp)]
        L.unc_model_acc_free.argtypes = [vp]; L.unc_model_acc_free.restype = None
        L.unc_model_acc_reset.argtypes = [vp]
        L.unc_model_acc_add.argtypes = [vp, u64, vp, vp, vp, vp]
        L.unc_model_acc_read.argtypes = [vp, vp, vp, vp, vp, C.POINTER(u64)]
        L.unc_model_acc_last_timing.argtypes = [C.POINTER(C.c_float)]
        L.unc_model_acc_finish.argtypes = [vp, vp, u32, C.POINTER(vp), C.POINTER(u32)]
        L.unc_align_call.argtypes = [C.POINTER(AlignCall)]
    if hasattr(L, "unc_pileup_create"):               # (with the alignment sources)
        L.unc_pileup_create.argtypes = [vp, u32, vp, u32, C.POINTER(vp)]
        L.unc_pileup_free.argtypes = [vp]; L.unc_pileup_free.restype = None
        L.unc_pileup_reset.argtypes = [vp]
        L.unc_pileup_device_bytes.argtypes = [vp]; L.unc_pileup_device_bytes.restype = u64
        L.unc_pileup_n_bins.argtypes = [vp]; L.unc_pileup_n_bins.restype = u64
        L.unc_pileup_counters.argtypes = [vp, C.POINTER(u64), C.POINTER(u64), C.POINTER(u64)]
        L.unc_pileup_add.argtypes = [vp, u64, vp, vp, vp, vp, vp, vp, vp]
        L.unc_align_pileup_call.argtypes = [C.POINTER(AlignCall), vp]
        L.unc_pileup_last_timing.argtypes = [C.POINTER(C.c_float)]
        L.unc_pileup_covered.argtypes = [vp, vp, u64, vp, u64, C.POINTER(u64)]
        L.unc_pileup_covered_last_timing.argtypes = [vp]
        L.unc_pileup_gather.argtypes = [vp, u64, vp, vp]
        L.unc_pileup_bin_locate.argtypes = [vp, u64, vp, vp, vp, vp]
        L.unc_pileup_merge.argtypes = [vp, vp]
        L.unc_pileup_stats.argtypes = [vp, vp, u64, vp, vp]
        L.unc_pileup_compare.argtypes = [vp, vp, u64, vp, vp]
    if hasattr(L, "unc_pileup_hist_enable"):
        L.unc_pileup_hist_enable.argtypes = [vp, vp, C.c_float]
        L.unc_pileup_hist_gather.argtypes = [vp, u64, vp, vp]
        L.unc_pileup_hist_centres.argtypes = [vp, u64, vp, vp]
        L.unc_pileup_ks.argtypes = [vp, vp, u64, vp, vp]
        L.unc_pileup_ks_last_timing.argtypes = [C.POINTER(C.c_float)]
    if hasattr(L, "unc_mask_create"):                 # (the emulator builds of the other features do not hold the masking entry points)
        L.unc_mask_create.argtypes = [C.c_int, vp, u64, vp, u32, C.POINTER(vp)]
        L.unc_mask_free.argtypes = [vp]; L.unc_mask_free.restype = None
        L.unc_mask_kmer_counts.argtypes = [vp, u32, vp]
        L.unc_mask_internal.argtypes = [vp, u32, u32, vp, vp, vp, C.POINTER(u32)]
        L.unc_mask_external.argtypes = [vp, vp, u32, u32, vp, C.POINTER(u64)]
        L.unc_mask_codes.argtypes = [vp, vp]
        L.unc_mask_last_timing.argtypes = [C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float)]
    _libs[key] = L
    return L


def _check(L, rc, allow=()):
    if rc != UNC_OK and rc not in allow:
        raise UncalledHipError(f"uncalled_hip error {rc}: {L.unc_last_error().decode()}")
    return rc


def default_params(lib=None):
    p = Params()
    (lib or load()).unc_params_default(C.byref(p))
    return p


class Model:
    """A pore model (unc_model_t): 1024 (level_mean, level_stdv) pairs in k-mer order.  PoreModel of the reference (pore_model.hpp)."""

    def __init__(self, handle, lib):
        self.L, self.h = lib, handle

    @classmethod
    def _made(cls, L, call, *args):
        h = C.c_void_p()
        _check(L, call(*args, C.byref(h)))
        return cls(h, L)

    @classmethod
    def default(cls, lib=None):
        """the compiled-in r9.4 template model"""
        L = lib or load()
        return cls._made(L, L.unc_model_default)

    @classmethod
    def load(cls, path, lib=None):
        """a file as the reference's r94_5mers.txt: a header line, then `kmer mean stdv` for all 1024 k-mers in any order"""
        L = lib or load()
        return cls._made(L, L.unc_model_load, str(path).encode())

    @classmethod
    def from_pairs(cls, pairs, lib=None):
        """pairs: float32 (1024, 2), or 2048 flat: mean and stdv of every k-mer"""
        L = lib or load()
        p = np.ascontiguousarray(pairs, dtype=np.float32).ravel()
        if p.size != 2048:
            raise ValueError("1024 (mean, stdv) pairs are needed")
        return cls._made(L, L.unc_model_from_pairs, p.ctypes.data)

    def close(self):
        if getattr(self, "h", None):
            self.L.unc_model_free(self.h)
            self.h = None

    __del__ = close

    def save(self, path):
        _check(self.L, self.L.unc_model_save(self.h, str(path).encode()))

    def pairs(self):
        out = np.empty((1024, 2), dtype=np.float32)
        _check(self.L, self.L.unc_model_pairs(self.h, out.ctypes.data))
        return out

    def tables(self, cmpl):
        """(means, vars_x2, lognorm, model_mean, model_stdv); cmpl=True: complemented, as Index.model_tables(); False: as dtw_model_tables()"""
        a, b, c = (np.empty(1024, dtype=np.float32) for _ in range(3))
        mm, ms = C.c_float(), C.c_float()
        _check(self.L, self.L.unc_model_tables(self.h, 1 if cmpl else 0, a.ctypes.data, b.ctypes.data, c.ctypes.data, C.byref(mm), C.byref(ms)))
        return a, b, c, mm.value, ms.value


class ModelAcc:
    """A training accumulator on one device (unc_model_acc_t): per k-mer n, S = sum q, SS = sum q * q, q = rint(level * 2^20), all
    integers.  Filled by add() or by align_batch / align_ref_batch with accumulate=; finish() makes the Model."""

    def __init__(self, device=0, keep_shared=False, lib=None):
        self.L = lib or load()
        h = C.c_void_p()
        _check(self.L, self.L.unc_model_acc_create(int(device), MODEL_KEEP_SHARED if keep_shared else 0, C.byref(h)))
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.L.unc_model_acc_free(self.h)
            self.h = None

    __del__ = close

    def add(self, kmers, levels, shared=None, stream=None):
        km = np.ascontiguousarray(kmers, dtype=np.uint16).ravel()
        lv = np.ascontiguousarray(levels, dtype=np.float32).ravel()
        sh = None if shared is None else np.ascontiguousarray(shared, dtype=np.uint32).ravel()
        if km.size != lv.size or (sh is not None and sh.size != km.size):
            raise ValueError("as many levels (and shared flags) as k-mers are needed")
        _check(self.L, self.L.unc_model_acc_add(self.h, km.size, km.ctypes.data, lv.ctypes.data, None if sh is None else sh.ctypes.data, stream))

    def read(self):
        """-> (n uint64[1024], S int64[1024], SS_lo uint64[1024], SS_hi uint64[1024], n_dropped)"""
        n, lo, hi = (np.empty(1024, dtype=np.uint64) for _ in range(3))
        S = np.empty(1024, dtype=np.int64)
        dropped = C.c_uint64()
        _check(self.L, self.L.unc_model_acc_read(self.h, n.ctypes.data, S.ctypes.data, lo.ctypes.data, hi.ctypes.data, C.byref(dropped)))
        return n, S, lo, hi, dropped.value

    def reset(self):
        _check(self.L, self.L.unc_model_acc_reset(self.h))

    def finish(self, prior=None, min_obs=2):
        """-> (Model, k-mers kept from the prior): a k-mer with fewer than max(min_obs, 2) records, or without spread, keeps the
        prior's pair (None: the r9.4 template's)"""
        h, kept = C.c_void_p(), C.c_uint32()
        _check(self.L, self.L.unc_model_acc_finish(self.h, prior.h if prior is not None else None, int(min_obs), C.byref(h), C.byref(kept)))
        return Model(h, self.L), kept.value

    def last_timing(self):
        """kernel milliseconds of k_model_accum in the calling thread's last add() or alignment call"""
        ms = C.c_float()
        self.L.unc_model_acc_last_timing(C.byref(ms))
        return ms.value


class Index:
    """Device-resident FM index + thresholds + pore model (Mapper::load_static, mapper.cpp:109-159)."""

    def __init__(self, prefix, preset="default", device=0, lib=None, dense_sa=True):
        """dense_sa=False: without the dense suffix array (UNC_INDEX_NO_DENSE_SA), for callers that only step through the BWT"""
        self.L = lib or load()
        h = C.c_void_p()
        if dense_sa:
            _check(self.L, self.L.unc_index_load(str(prefix).encode(), preset.encode(), device, C.byref(h)))
        else:
            _check(self.L, self.L.unc_index_load_flags(str(prefix).encode(), preset.encode(), device, INDEX_NO_DENSE_SA, C.byref(h)))
        self.h = h
        self.size = self.L.unc_index_size(h)

    def close(self):
        if getattr(self, "h", None):
            self.L.unc_index_free(self.h)
            self.h = None

    __del__ = close

    def seq_names(self):
        return [self.L.unc_index_seq_name(self.h, i).decode() for i in range(self.L.unc_index_n_seqs(self.h))]

    def seq_len(self, rid):
        return self.L.unc_index_seq_len(self.h, rid)

    def device_bytes(self):
        return self.L.unc_index_device_bytes(self.h)

    def kmer_ranges(self):
        out = np.empty((1024, 2), dtype=np.uint64)
        self.L.unc_index_kmer_ranges(self.h, out.ctypes.data)
        return out

    def thresholds(self):
        out = np.empty(64, dtype=np.float32)
        self.L.unc_index_thresholds(self.h, out.ctypes.data)
        return out

    def model_tables(self):
        a, b, c = (np.empty(1024, dtype=np.float32) for _ in range(3))
        mm, ms = C.c_float(), C.c_float()
        self.L.unc_index_model_tables(self.h, a.ctypes.data, b.ctypes.data, c.ctypes.data, C.byref(mm), C.byref(ms))
        return a, b, c, mm.value, ms.value

    def set_model(self, model):
        """unc_index_set_model: the index maps with `model` from now on; refused once a Mapper or Realtime was made from the index"""
        _check(self.L, self.L.unc_index_set_model(self.h, model.h))

    def get_neighbor(self, starts, ends, bases):
        s = np.ascontiguousarray(starts, dtype=np.uint64)
        e = np.ascontiguousarray(ends, dtype=np.uint64)
        b = np.ascontiguousarray(bases, dtype=np.uint8)
        os_, oe = np.empty_like(s), np.empty_like(s)
        _check(self.L, self.L.unc_fm_get_neighbor(self.h, s.size, s.ctypes.data, e.ctypes.data, b.ctypes.data,
                                                  os_.ctypes.data, oe.ctypes.data))
        return os_, oe

    def sa(self, rows):
        r = np.ascontiguousarray(rows, dtype=np.uint64)
        out = np.empty_like(r)
        _check(self.L, self.L.unc_fm_sa(self.h, r.size, r.ctypes.data, out.ctypes.data))
        return out

    def self_align(self, prefix, sample_dist, cap=128):
        """self_align(bwa_prefix, sample_dist) of the reference: (lens uint64[n, cap], full_len uint32[n])."""
        n = C.c_uint64()
        _check(self.L, self.L.unc_self_align(self.h, str(prefix).encode(), sample_dist, cap, None, None, 0, C.byref(n)))
        lens = np.zeros((n.value, cap), dtype=np.uint64)
        full = np.zeros(n.value, dtype=np.uint32)
        _check(self.L, self.L.unc_self_align(self.h, str(prefix).encode(), sample_dist, cap, lens.ctypes.data, full.ctypes.data,
                                             n.value, C.byref(n)))
        return lens, full

    def match_probs(self, levels):
        lv = np.ascontiguousarray(levels, dtype=np.float32)
        out = np.empty((lv.size, 1024), dtype=np.float32)
        _check(self.L, self.L.unc_match_probs(self.h, lv.size, lv.ctypes.data, out.ctypes.data))
        return out


def dtw_model_tables(lib=None):
    """Host copies of the r9.4 TEMPLATE model's tables the DTW costs read: (means, vars_x2, lognorm), 1024 float32 each."""
    L = lib or load()
    a, b, c = (np.empty(1024, dtype=np.float32) for _ in range(3))
    L.unc_dtw_model_tables(a.ctypes.data, b.ctypes.data, c.ctypes.data)
    return a, b, c


def dtw_batch(events_list, kmers_list, params, workspace_bytes=0, paths=True, device=0, stream=None, lib=None, full=False, band=0, model=None,
              adaptive=0):
    """unc_dtw_batch: DTWr94p / DTWr94d (dtw.hpp) of events_list[a] (columns) against kmers_list[a] (rows) for every a, on the GPU.
    -> (scores float32[n], mean scores float32[n], paths): paths[a] is DTW::get_path() as an (len, 2) uint32 array of (event, k-mer)
    pairs, end cell first (None with paths=False, and for an alignment that was not computed: status DTW_TOO_LARGE or
    DTW_BAND_TOO_NARROW).  full=True returns the DTW_RESULT records (score, mean_score, path_len, status) in place of the first two.
    band=W > 0: unc_dtw_band_batch, the same within a band of half-width W around the diagonal (global alignment only); with
    status DTW_LEFT_BAND paths[a] holds the pairs up to the last cell in the band.  model: a Model whose tables the costs read
    (unc_dtw_model_batch; None: the r9.4 template).  adaptive=B (64, 128 or 256): unc_dtw_adapt_batch, a band of B rows that follows
    the path from (0, 0) to an open end in the last column; status DTW_REF_END: the end cell lies in the last row."""
    L = lib or load()
    if adaptive and (band or model is not None):
        raise ValueError("adaptive= goes with neither band= nor model=")
    n = len(events_list)
    if n != len(kmers_list):
        raise ValueError("as many k-mer arrays as event arrays are needed")
    evs = [np.ascontiguousarray(e, dtype=np.float32).ravel() for e in events_list]
    kms = [np.ascontiguousarray(k, dtype=np.uint16).ravel() for k in kmers_list]
    ev_off = np.cumsum([0] + [e.size for e in evs]).astype(np.uint64)
    km_off = np.cumsum([0] + [k.size for k in kms]).astype(np.uint64)
    ev = np.concatenate(evs) if n else np.zeros(0, np.float32)
    km = np.concatenate(kms) if n else np.zeros(0, np.uint16)
    if ev.size == 0:
        ev = np.zeros(1, np.float32)        # (a valid address for the library's own argument checks)
    if km.size == 0:
        km = np.zeros(1, np.uint16)
    res = np.zeros(n, dtype=DTW_RESULT)
    path = path_off = None
    if paths:
        path_off = np.cumsum([0] + [max(0, e.size + k.size - 1) for e, k in zip(evs, kms)]).astype(np.uint64)
        path = np.empty((max(1, int(path_off[-1])), 2), dtype=np.uint32)
    args = (int(workspace_bytes), res.ctypes.data, path.ctypes.data if paths else None, path_off.ctypes.data if paths else None, stream)
    if adaptive:
        _check(L, L.unc_dtw_adapt_batch(int(device), n, ev.ctypes.data, ev_off.ctypes.data, km.ctypes.data, km_off.ctypes.data,
                                        C.byref(params), int(adaptive), *args))
    elif model is not None:
        _check(L, L.unc_dtw_model_batch(int(device), model.h, n, ev.ctypes.data, ev_off.ctypes.data, km.ctypes.data, km_off.ctypes.data,
                                        C.byref(params), int(band), *args))
    elif band:
        _check(L, L.unc_dtw_band_batch(int(device), n, ev.ctypes.data, ev_off.ctypes.data, km.ctypes.data, km_off.ctypes.data,
                                       C.byref(params), int(band), *args))
    else:
        _check(L, L.unc_dtw_batch(int(device), n, ev.ctypes.data, ev_off.ctypes.data, km.ctypes.data, km_off.ctypes.data, C.byref(params),
                                  *args))
    out_paths = None
    if paths:
        out_paths = [None if res["status"][a] in (DTW_TOO_LARGE, DTW_BAND_TOO_NARROW) else path[int(path_off[a]):int(path_off[a]) + int(res["path_len"][a])].copy()
                     for a in range(n)]
    if full:
        return res, out_paths
    return res["score"].copy(), res["mean_score"].copy(), out_paths


def dtw_last_timing(lib=None):
    """(kernel milliseconds, rounds, bytes of back-pointers held at most) of the calling thread's last dtw_batch, with or without a band."""
    L = lib or load()
    ms, rounds, nbytes = C.c_float(), C.c_uint32(), C.c_uint64()
    L.unc_dtw_last_timing(C.byref(ms), C.byref(rounds), C.byref(nbytes))
    return ms.value, rounds.value, nbytes.value


def align_opts(dtw=None, mask=True, create_events=True, target="kmers", max_events=0, band=0, adaptive=0):
    """AlignOpts from words: dtw = a DTWParams (None: dtw_test's), target = "kmers" | "model", band = the DTW's half-width (0: the
    full matrix), adaptive = the width B of the adaptive band with an open end (in place of band)."""
    if target not in ("kmers", "model"):
        raise ValueError("target is 'kmers' or 'model'")
    if adaptive and band:
        raise ValueError("adaptive= and band= exclude each other")
    o = AlignOpts()
    o.flags = (ALIGN_DTW_PARAMS if dtw is not None else 0) | (0 if mask else ALIGN_NO_MASK) | (0 if create_events else ALIGN_RAW) | \
        (ALIGN_TARGET_MODEL if target == "model" else 0) | (ALIGN_ADAPTIVE if adaptive else 0)
    o.max_events = int(max_events)
    o.band = int(adaptive) if adaptive else int(band)
    if dtw is not None:
        o.dtw = dtw
    return o


class _SegOut:
    """the buffers behind segments=True / events=True of align_batch and align_ref_batch: room for every k-mer of a query and for every
    column it can have"""

    def __init__(self, n_kmers, col_room, segments, events):
        n = len(n_kmers)
        self.segments, self.events = segments, events
        self.arg = AlignSegments()
        if segments:
            self.seg_off = np.cumsum([0] + list(n_kmers)).astype(np.uint64)
            self.seg = np.zeros(max(1, int(self.seg_off[-1])), dtype=SEGMENT)
            self.info = np.zeros(n, dtype=SEG_INFO)
            self.arg.seg, self.arg.seg_off, self.arg.info = self.seg.ctypes.data, self.seg_off.ctypes.data, self.info.ctypes.data
        if events:
            self.evt_off = np.cumsum([0] + list(col_room)).astype(np.uint64)
            self.evt = np.zeros(max(1, int(self.evt_off[-1])), dtype=EVENT)
            self.arg.events, self.arg.evt_off = self.evt.ctypes.data, self.evt_off.ctypes.data

    def results(self, res):
        """what the call returns after its other outputs: with segments a list of SEGMENT arrays per query and the SEG_INFO records
        (row_first, n_rows, status), with events a list of EVENT arrays (a query's columns)"""
        out = []
        if self.segments:
            out.append([self.seg[int(self.seg_off[q]):int(self.seg_off[q]) + int(self.info["n_rows"][q])].copy() for q in range(len(res))])
            out.append(self.info)
        if self.events:
            out.append([self.evt[int(self.evt_off[q]):int(self.evt_off[q]) + int(res["n_kept"][q])].copy() for q in range(len(res))])
        return out


def _align(L, entries, first, rows_args, n_rows, tap_args, tap, raw, offsets, calib, queries, opts, params, workspace_bytes, levels, paths,
           on_device, stream, segments, events, model=None, accumulate=None, rec_rows=None, pileup=None):
    """what align_batch and align_ref_batch share: the ALIGN_QUERY records, raw on the host or the device, the room per query, the buffers
    of levels and paths, _SegOut, the call and the tuple it returns.  entries: the entry point's name without and with segments;
    first: its first argument; rows_args: what names the rows, after the queries; n_rows: the rows of every query; tap_args: what
    follows lev_off; tap: None, or what makes the list that goes between the paths and the segments' outputs.  With a model or an
    accumulator the call goes through unc_align_call: rec_rows are then the fields of its record that name the rows; with a pile-up
    through unc_align_pileup_call, with the same record"""
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    calib = np.ascontiguousarray(calib, dtype=CALIB)
    n_reads, n = offsets.size - 1, len(queries)
    qs = np.zeros(n, dtype=ALIGN_QUERY)
    for i, (r, st, en) in enumerate(queries):
        qs[i]["read"], qs[i]["smp_st"], qs[i]["smp_en"] = r, st, en
    if on_device:
        raw_ptr = int(raw)
    else:
        raw = np.ascontiguousarray(raw, dtype=np.int16)
        raw_ptr = raw.ctypes.data
    res = np.zeros(n, dtype=ALIGN_RESULT)
    # room per query: what a slice can give at most (n / 2 + 16 events; its samples without events); a bad slice is the library's to refuse
    room = []
    for r, st, en in queries:
        ln = int(offsets[r + 1] - offsets[r]) if 0 <= r < n_reads else 0
        ns = max(0, (int(en) if en else ln) - int(st))
        room.append(ns if opts is not None and opts.flags & ALIGN_RAW else ns // 2 + 16)
    lev = lev_off = path = path_off = None
    if levels:
        lev_off = np.cumsum([0] + room).astype(np.uint64)
        lev = np.empty(max(1, int(lev_off[-1])), dtype=np.float32)
    if paths:
        path_off = np.cumsum([0] + [max(0, c + k - 1) for c, k in zip(room, n_rows)]).astype(np.uint64)
        path = np.empty((max(1, int(path_off[-1])), 2), dtype=np.uint32)
    args = (first, C.byref(params) if params is not None else None, C.byref(opts) if opts is not None else None,
            n_reads, raw_ptr, offsets.ctypes.data, calib.ctypes.data, 1 if on_device else 0, n, qs.ctypes.data,
            *rows_args, int(workspace_bytes), res.ctypes.data,
            lev.ctypes.data if levels else None, lev_off.ctypes.data if levels else None, *tap_args,
            path.ctypes.data if paths else None, path_off.ctypes.data if paths else None)
    so = _SegOut(n_rows, room, segments, events) if segments or events else None
    if model is not None or accumulate is not None or pileup is not None:
        rec = AlignCall()
        rec.size = C.sizeof(AlignCall)
        rec.params = C.cast(C.pointer(params), C.c_void_p) if params is not None else None
        rec.opts = C.cast(C.pointer(opts), C.c_void_p) if opts is not None else None
        rec.n_reads, rec.on_device, rec.raw, rec.offsets, rec.calib = n_reads, 1 if on_device else 0, raw_ptr, offsets.ctypes.data, calib.ctypes.data
        rec.n_queries, rec.queries, rec.workspace_bytes, rec.results = n, qs.ctypes.data, int(workspace_bytes), res.ctypes.data
        rec.levels, rec.lev_off = (lev.ctypes.data, lev_off.ctypes.data) if levels else (None, None)
        rec.path, rec.path_off = (path.ctypes.data, path_off.ctypes.data) if paths else (None, None)
        rec.segs = C.cast(C.pointer(so.arg), C.c_void_p) if so is not None else None
        rec.model = model.h if model is not None else None
        rec.accumulate = accumulate.h if accumulate is not None else None
        rec.stream = stream
        for k, v in rec_rows.items():
            setattr(rec, k, v)
        _check(L, L.unc_align_call(C.byref(rec)) if pileup is None else L.unc_align_pileup_call(C.byref(rec), pileup.h))
    elif so is not None:
        _check(L, getattr(L, entries[1])(*args, C.byref(so.arg), stream))
    else:
        _check(L, getattr(L, entries[0])(*args, stream))
    out = [res]
    if levels:
        out.append([lev[int(lev_off[q]):int(lev_off[q]) + int(res["n_kept"][q])].copy() for q in range(n)])
    if paths:
        done = (DTW_OK, DTW_PATH_TRUNCATED, DTW_LEFT_BAND, DTW_REF_END)
        out.append([path[int(path_off[q]):int(path_off[q]) + int(res["dtw"]["path_len"][q])].copy() if res["status"][q] in done else None
                    for q in range(n)])
    if tap is not None:
        out.append(tap())
    if so is not None:
        out += so.results(res)
    return out[0] if len(out) == 1 else tuple(out)


def align_batch(raw, offsets, calib, queries, kmers_list, opts=None, params=None, workspace_bytes=0, levels=False, paths=False,
                on_device=False, device=0, stream=None, lib=None, segments=False, events=False, model=None, accumulate=None, pileup=None):
    """unc_align_batch: the pipeline of the reference's dtw_test (slice -> events -> stall mask -> normalisation to the k-mers'
    levels -> DTW) for a batch of queries on the GPU.  raw / offsets / calib: the reads as Mapper.map_batch takes them (raw: an int16
    array, or with on_device=True a device address).  queries: (read index, smp_st, smp_en) triples, smp_en == 0 = to the read's end;
    kmers_list[q]: query q's reference k-mers.  -> ALIGN_RESULT records (dtw.score, dtw.mean_score, dtw.path_len, n_events, n_kept,
    tgt_mean, tgt_stdv, scale, shift, status); with levels=True and / or paths=True also a list of the normalised columns per query and
    a list of paths as dtw_batch returns them (None for a query that was not aligned).  segments=True (unc_align_segments_batch): then
    also a list of SEGMENT arrays -- per query one record per k-mer on its path, in the read's sample coordinates -- and the SEG_INFO
    records (row_first, n_rows, status); events=True: then also a list of EVENT arrays, the query's columns as events.
    model: a Model in place of the r9.4 template (costs and targets); accumulate: a ModelAcc that receives every record of the
    alignments' paths, asked for or not (unc_align_call).  pileup: refused -- k-mer arrays have no coordinates (align_ref_batch)."""
    if pileup is not None:
        raise ValueError("a pile-up needs coordinates: use align_ref_batch")
    if len(queries) != len(kmers_list):
        raise ValueError("as many k-mer arrays as queries are needed")
    kms = [np.ascontiguousarray(k, dtype=np.uint16).ravel() for k in kmers_list]
    km_off = np.cumsum([0] + [k.size for k in kms]).astype(np.uint64)
    km = np.concatenate(kms + [np.zeros(1, np.uint16)])         # (one element more: a valid address for the library's own argument checks)
    return _align(lib or load(), ("unc_align_batch", "unc_align_segments_batch"), int(device), (km.ctypes.data, km_off.ctypes.data),
                  [k.size for k in kms], (), None, raw, offsets, calib, queries, opts, params, workspace_bytes, levels, paths, on_device, stream,
                  segments, events, model, accumulate, dict(device=int(device), kmers=km.ctypes.data, km_off=km_off.ctypes.data))


def align_segments_last_timing(lib=None):
    """kernel milliseconds of k_align_segments in the calling thread's last alignment call, summed over the DTW's rounds"""
    L = lib or load()
    ms = C.c_float()
    L.unc_align_segments_last_timing(C.byref(ms))
    return ms.value


def align_last_timing(lib=None):
    """kernel milliseconds of the calling thread's last align_batch: (slices gathered, event detection, mask + target + normalisation, DTW)."""
    L = lib or load()
    ms = np.zeros(4, np.float32)
    L.unc_align_last_timing(ms.ctypes.data)
    return tuple(float(x) for x in ms)


def align_model_target(lib=None):
    """(mean, stdv) of the r9.4 template model's levels over all k-mers: the target of target="model"."""
    L = lib or load()
    a, b = C.c_float(), C.c_float()
    L.unc_align_model_target(C.byref(a), C.byref(b))
    return np.float32(a.value), np.float32(b.value)


def ref_kmers(index, prefix, rid, st, en, fwd=True):
    """BwaIndex::get_kmers (bwa_index.hpp:247-255): the 5-mers of bases [st, en) of sequence rid, read from <prefix>.pac;
    fwd=False: kmers_revcomp of them (bp.hpp:82-99).  Host only."""
    L = index.L
    n = C.c_uint64()
    _check(L, L.unc_ref_kmers(index.h, str(prefix).encode(), int(rid), int(st), int(en), 1 if fwd else 0, None, 0, C.byref(n)))
    out = np.empty(n.value, dtype=np.uint16)
    if n.value:
        _check(L, L.unc_ref_kmers(index.h, str(prefix).encode(), int(rid), int(st), int(en), 1 if fwd else 0, out.ctypes.data, out.size, C.byref(n)))
    return out


class RefSeq:
    """unc_refseq_t: the packed reference <prefix>.pac, read once, kept on the host and in HBM beside the index
    (BwaIndex::load_pacseq).  Close it before the index it was loaded for (it keeps a reference to the index, so garbage collection
    takes them in that order)."""

    def __init__(self, index, prefix):
        self.index = index
        self.L = index.L
        h = C.c_void_p()
        _check(self.L, self.L.unc_refseq_load(index.h, str(prefix).encode(), C.byref(h)))
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.L.unc_refseq_free(self.h)
            self.h = None

    __del__ = close

    def device_bytes(self):
        return self.L.unc_refseq_device_bytes(self.h)


class Masker:
    """unc_mask_t: a reference as one code per base (0..3 = ACGT, 4 = not a base) with its contig offsets, resident on the GPU, and
    the two masking recipes of the reference's masking/ directory run on it in place (include/uncalled_hip.h).  A context manager:

        with capi.Masker(codes, offsets) as m:
            report = m.internal(10, 30)
            masked = m.codes()
    """

    def __init__(self, codes, ctg_off, device=0, lib=None):
        self.L = lib or load()
        codes = np.ascontiguousarray(codes, dtype=np.uint8)
        off = np.ascontiguousarray(ctg_off, dtype=np.uint64)
        if off.size < 1:
            raise ValueError("the contig offsets hold at least the 0 they start from")
        self.n = int(codes.size)
        h = C.c_void_p()
        _check(self.L, self.L.unc_mask_create(device, codes.ctypes.data, self.n, off.ctypes.data, off.size - 1, C.byref(h)))
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.L.unc_mask_free(self.h)
            self.h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def kmer_counts(self, k):
        """the count of every k-mer's windows in the text as it stands -> uint32[4^k] (UncalledHipError for k outside 1..13)"""
        out = np.zeros(4 ** k if 1 <= k <= 13 else 1, dtype=np.uint32)
        _check(self.L, self.L.unc_mask_kmer_counts(self.h, k, out.ctypes.data))
        return out

    def internal(self, k, iters):
        """mask_internal.sh: -> [(k-mer code, occurrences, bases newly masked)] per iteration done (fewer than iters when no k-mer
        is left that occurs twice)"""
        room = max(1, int(iters))
        km, occ, bases = (np.zeros(room, dtype=np.uint32) for _ in range(3))
        done = C.c_uint32()
        _check(self.L, self.L.unc_mask_internal(self.h, k, iters, km.ctypes.data, occ.ctypes.data, bases.ctypes.data, C.byref(done)))
        return [(int(km[i]), int(occ[i]), int(bases[i])) for i in range(done.value)]

    def external(self, index, min_len, min_copy, counts=False):
        """mask_external.sh against a loaded capi.Index on the same device -> bases newly masked, and with counts=True the count of
        the window that starts at every position (uint64, 0 where there is none) as well"""
        tap = np.zeros(max(1, self.n), dtype=np.uint64) if counts else None
        masked = C.c_uint64()
        _check(self.L, self.L.unc_mask_external(self.h, index.h, min_len, min_copy, tap.ctypes.data if counts else None, C.byref(masked)))
        return (masked.value, tap[:self.n]) if counts else masked.value

    def codes(self):
        out = np.empty(max(1, self.n), dtype=np.uint8)
        _check(self.L, self.L.unc_mask_codes(self.h, out.ctypes.data))
        return out[:self.n]

    def last_timing(self):
        """kernel milliseconds of the calling thread's last call: (counting and choosing, flagging and covering, FM look-ups)"""
        a, b, c = C.c_float(), C.c_float(), C.c_float()
        self.L.unc_mask_last_timing(C.byref(a), C.byref(b), C.byref(c))
        return a.value, b.value, c.value


def _stretches(stretches):
    """(rid, st, en, fwd) tuples -> REF_STRETCH records"""
    out = np.zeros(len(stretches), dtype=REF_STRETCH)
    for i, (rid, st, en, fwd) in enumerate(stretches):
        out[i]["rid"], out[i]["st"], out[i]["en"], out[i]["fwd"] = rid, st, en, 1 if fwd else 0
    return out


def ref_kmers_batch(refseq, stretches, stream=None):
    """unc_refseq_kmers_batch: BwaIndex::get_kmers for a batch of (rid, st, en, fwd) stretches in one kernel launch on the GPU
    -> a list of uint16 arrays, what ref_kmers gives for each (empty below five bases)."""
    L = refseq.L
    ss = _stretches(stretches)
    counts = [max(0, int(en) - int(st) - 4) for _, st, en, _ in stretches]
    off = np.cumsum([0] + counts).astype(np.uint64)
    out = np.empty(max(1, int(off[-1])), dtype=np.uint16)
    _check(L, L.unc_refseq_kmers_batch(refseq.h, len(stretches), ss.ctypes.data, out.ctypes.data, off.ctypes.data, stream))
    return [out[int(off[a]):int(off[a + 1])].copy() for a in range(len(stretches))]


def align_ref_batch(refseq, raw, offsets, calib, queries, stretches, opts=None, params=None, workspace_bytes=0, levels=False, paths=False,
                    kmers=False, on_device=False, stream=None, segments=False, events=False, model=None, accumulate=None, pileup=None):
    """unc_align_ref_batch: align_batch with coordinates in place of k-mer arrays.  stretches[q] = (rid, st, en, fwd) names the bases
    whose k-mers are query q's rows; they are made on the GPU (the index's) and reach the host only with kmers=True.  Everything else
    as align_batch, and so are the results, bit for bit, for the k-mers ref_kmers gives for the same stretches.  -> ALIGN_RESULT
    records, then, as asked for, the lists of levels, of paths and of k-mers per query, and what segments=True / events=True add
    (unc_align_ref_segments_batch; as in align_batch, after everything else).  model, accumulate: as in align_batch.  pileup: a Pileup of
    this refseq that receives every record of the alignments' paths at its reference position, asked for or not (unc_align_pileup_call)."""
    if len(queries) != len(stretches):
        raise ValueError("as many stretches as queries are needed")
    ss = _stretches(stretches)
    counts = [max(0, int(en) - int(st) - 4) for _, st, en, _ in stretches]
    km_off = np.cumsum([0] + counts).astype(np.uint64)
    km = np.empty(max(1, int(km_off[-1])), dtype=np.uint16) if kmers else None
    return _align(refseq.L, ("unc_align_ref_batch", "unc_align_ref_segments_batch"), refseq.h, (ss.ctypes.data,), counts,
                  (km.ctypes.data, km_off.ctypes.data) if kmers else (None, None),
                  (lambda: [km[int(km_off[q]):int(km_off[q + 1])].copy() for q in range(len(counts))]) if kmers else None,
                  raw, offsets, calib, queries, opts, params, workspace_bytes, levels, paths, on_device, stream, segments, events, model,
                  accumulate, dict(refseq=refseq.h, stretches=ss.ctypes.data, kmers_out=km.ctypes.data if kmers else None,
                                   kmers_off=km_off.ctypes.data if kmers else None), pileup)


class Pileup:
    """A signal pile-up on the device of a RefSeq (unc_pileup_t): per bin = (reference position of a 5-mer's leftmost base, strand) the
    integer sums n, S = sum q, SS = sum q * q (128 bits), D = sum of dwell samples over the records of many alignments,
    q = rint(level * 2^20).  regions: (rid, st, en) triples (None: every sequence, whole); the bins are numbered in the regions' sorted
    order, by position, then strand (plus first).  Filled by add() or by align_ref_batch with pileup=.  Close it before its RefSeq (it
    keeps a reference to it, so garbage collection takes them in that order)."""

    def __init__(self, refseq, regions=None, keep_shared=False, lib=None):
        self.refseq = refseq
        self.L = lib or refseq.L
        rg = None if regions is None else _stretches([(rid, st, en, True) for rid, st, en in regions])
        h = C.c_void_p()
        _check(self.L, self.L.unc_pileup_create(refseq.h, 0 if rg is None else len(rg), None if rg is None else rg.ctypes.data,
                                                PILEUP_KEEP_SHARED if keep_shared else 0, C.byref(h)))
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.L.unc_pileup_free(self.h)
            self.h = None

    __del__ = close

    def n_bins(self):
        return int(self.L.unc_pileup_n_bins(self.h))

    def device_bytes(self):
        return int(self.L.unc_pileup_device_bytes(self.h))

    def add(self, rid, pos, fwd, level, smp_n, shared=None, stream=None):
        """records from host arrays: sequence, position, strand (non-zero: plus), normalised level, dwell samples, shared flag"""
        r = np.ascontiguousarray(rid, dtype=np.int32).ravel()
        p = np.ascontiguousarray(pos, dtype=np.uint64).ravel()
        f = np.ascontiguousarray(fwd, dtype=np.uint32).ravel()
        lv = np.ascontiguousarray(level, dtype=np.float32).ravel()
        d = np.ascontiguousarray(smp_n, dtype=np.uint32).ravel()
        sh = None if shared is None else np.ascontiguousarray(shared, dtype=np.uint32).ravel()
        if not (r.size == p.size == f.size == lv.size == d.size) or (sh is not None and sh.size != r.size):
            raise ValueError("the records' arrays must be equally long")
        _check(self.L, self.L.unc_pileup_add(self.h, r.size, r.ctypes.data, p.ctypes.data, f.ctypes.data, lv.ctypes.data, d.ctypes.data,
                                             None if sh is None else sh.ctypes.data, stream))

    def reset(self):
        _check(self.L, self.L.unc_pileup_reset(self.h))

    def counters(self):
        """-> (n_dropped, n_outside, n_added)"""
        a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
        _check(self.L, self.L.unc_pileup_counters(self.h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def covered(self, min_cov, other=None, cap=None):
        """the bins with at least min_cov records (in `other` as well, if given), ascending -> uint64 array; with cap (the first cap
        of them) -> (array, full count)"""
        n = C.c_uint64()
        room = self.n_bins() if cap is None else int(cap)
        out = np.empty(max(1, room), dtype=np.uint64)
        _check(self.L, self.L.unc_pileup_covered(self.h, other.h if other is not None else None, int(min_cov), out.ctypes.data, room, C.byref(n)))
        got = out[:min(room, n.value)].copy()
        return got if cap is None else (got, n.value)

    def covered_last_timing(self):
        """kernel milliseconds of the calling thread's last covered(): (counts, scan, write)"""
        ms = np.zeros(3, np.float32)
        self.L.unc_pileup_covered_last_timing(ms.ctypes.data)
        return tuple(float(x) for x in ms)

    def gather(self, bins):
        """the five words of the listed bins -> PILEUP_WORDS records (n, S, SS_lo, SS_hi, D)"""
        b = np.ascontiguousarray(bins, dtype=np.uint64).ravel()
        out = np.zeros(b.size, dtype=PILEUP_WORDS)
        _check(self.L, self.L.unc_pileup_gather(self.h, b.size, b.ctypes.data, out.ctypes.data))
        return out

    def locate(self, bins):
        """-> (rid int32, pos uint64, fwd uint32) of the listed bins"""
        b = np.ascontiguousarray(bins, dtype=np.uint64).ravel()
        rid, pos, fwd = np.zeros(b.size, np.int32), np.zeros(b.size, np.uint64), np.zeros(b.size, np.uint32)
        _check(self.L, self.L.unc_pileup_bin_locate(self.h, b.size, b.ctypes.data, rid.ctypes.data, pos.ctypes.data, fwd.ctypes.data))
        return rid, pos, fwd

    def stats(self, bins, model=None):
        """-> PILEUP_STAT records: kmer, n, mean, sd, dwell, the model's pair and z, exact (model None: the r9.4 template)"""
        b = np.ascontiguousarray(bins, dtype=np.uint64).ravel()
        out = np.zeros(b.size, dtype=PILEUP_STAT)
        _check(self.L, self.L.unc_pileup_stats(self.h, model.h if model is not None else None, b.size, b.ctypes.data, out.ctypes.data))
        return out

    def compare(self, other, bins):
        """-> PILEUP_CMP records: the two means and deviations, se2 and Welch's t; every listed bin needs two records in both"""
        b = np.ascontiguousarray(bins, dtype=np.uint64).ravel()
        out = np.zeros(b.size, dtype=PILEUP_CMP)
        _check(self.L, self.L.unc_pileup_compare(self.h, other.h, b.size, b.ctypes.data, out.ctypes.data))
        return out

    def merge(self, other):
        """adds `other` (same regions; any device) into this one"""
        _check(self.L, self.L.unc_pileup_merge(self.h, other.h))

    def last_timing(self):
        """kernel milliseconds of k_pileup_accum in the calling thread's last add() or alignment call"""
        ms = C.c_float()
        self.L.unc_pileup_last_timing(C.byref(ms))
        return ms.value

    def enable_hist(self, width, model=None):
        """attaches a level histogram to this (empty) pile-up: 64 buckets of `width` levels a bin, bucket 32 beginning at the model's
        mean for the bin's k-mer (model None: the r9.4 template).  Meant for regions: 256 bytes a bin"""
        _check(self.L, self.L.unc_pileup_hist_enable(self.h, model.h if model is not None else None, float(width)))

    def hist(self, bins):
        """the histograms of the listed bins -> uint32[n, 64]"""
        b = np.ascontiguousarray(bins, dtype=np.uint64).ravel()
        out = np.zeros((b.size, PILEUP_HIST_BUCKETS), dtype=np.uint32)
        _check(self.L, self.L.unc_pileup_hist_gather(self.h, b.size, b.ctypes.data, out.ctypes.data))
        return out

    def hist_centres(self, bins):
        """the centres of the listed bins' histograms, rint(model mean * 2^20) -> int64[n]"""
        b = np.ascontiguousarray(bins, dtype=np.uint64).ravel()
        out = np.zeros(b.size, dtype=np.int64)
        _check(self.L, self.L.unc_pileup_hist_centres(self.h, b.size, b.ctypes.data, out.ctypes.data))
        return out

    def ks(self, other, bins):
        """-> PILEUP_KS records: the two-sample Kolmogorov-Smirnov distance of this pile-up's and `other`'s histograms at the listed
        bins, exact (k_pileup_ks); every listed bin needs a record in both"""
        b = np.ascontiguousarray(bins, dtype=np.uint64).ravel()
        out = np.zeros(b.size, dtype=PILEUP_KS)
        _check(self.L, self.L.unc_pileup_ks(self.h, other.h, b.size, b.ctypes.data, out.ctypes.data))
        return out

    def ks_last_timing(self):
        """kernel milliseconds of k_pileup_ks in the calling thread's last ks()"""
        ms = C.c_float()
        self.L.unc_pileup_ks_last_timing(C.byref(ms))
        return ms.value


def align_ref_last_timing(lib=None):
    """kernel milliseconds of k_ref_kmers in the calling thread's last align_ref_batch"""
    L = lib or load()
    ms = C.c_float()
    L.unc_align_ref_last_timing(C.byref(ms))
    return ms.value


def make_calib(n, rng, offset, digitisation):
    c = np.empty(n, dtype=CALIB)
    c["range"], c["offset"], c["digitisation"] = rng, offset, digitisation
    return c


def hit_paf_cols(h, names):
    """PAF columns 2-12 (Paf::print_paf, read_buffer.cpp:92-118) of one HIT record."""
    if not h["mapped"]:
        return (int(h["rd_len"]), "*")
    name = names[int(h["rid"])] if h["rid"] >= 0 else ""
    return (int(h["rd_len"]), int(h["rd_st"]), int(h["rd_en"]), "+" if h["fwd"] else "-", name,
            int(h["rf_len"]), int(h["rf_st"]), int(h["rf_en"]), int(h["matches"]),
            int(h["rf_en"] - h["rf_st"] + 1), 255)


class Mapper:
    """Batch mapper: N x (Mapper::new_read + Mapper::map_read) on the GPU (mapper.cpp:188-207)."""

    def __init__(self, index, params=None, n_slots=0, max_clusters=0, max_seed_paths=0, slice_events=0, n_waves=0, pool_chunks=0,
                 events_reads_per_wave=0, sched_parts=0):
        self.index = index
        self.L = index.L
        self.params = params or default_params(self.L)
        opts = MapperOpts(n_slots, max_clusters, max_seed_paths, slice_events, n_waves, pool_chunks, sched_parts, events_reads_per_wave)
        h = C.c_void_p()
        _check(self.L, self.L.unc_mapper_create(index.h, C.byref(self.params), C.byref(opts), C.byref(h)))
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.L.unc_mapper_free(self.h)
            self.h = None

    __del__ = close

    def device_bytes(self):
        return self.L.unc_mapper_device_bytes(self.h)

    def map_batch(self, raw_i16, offsets_u64, calib, allow_overflow=False):
        """raw: host int16 array (all reads concatenated); returns HIT[n_reads]."""
        raw = np.ascontiguousarray(raw_i16, dtype=np.int16)
        off = np.ascontiguousarray(offsets_u64, dtype=np.uint64)
        cal = np.ascontiguousarray(calib, dtype=CALIB)
        n = off.size - 1
        hits = np.zeros(n, dtype=HIT)
        _check(self.L, self.L.unc_map_batch(self.h, n, raw.ctypes.data, off.ctypes.data, cal.ctypes.data, 0, None,
                                            hits.ctypes.data), allow=(UNC_ERR_OVERFLOW,) if allow_overflow else ())
        return hits

    def map_batch_device(self, raw_ptr, offsets_u64, calib, stream=None, allow_overflow=False):
        """raw_ptr: integer device address of the int16 samples already resident in HBM."""
        off = np.ascontiguousarray(offsets_u64, dtype=np.uint64)
        cal = np.ascontiguousarray(calib, dtype=CALIB)
        n = off.size - 1
        hits = np.zeros(n, dtype=HIT)
        _check(self.L, self.L.unc_map_batch(self.h, n, C.c_void_p(raw_ptr), off.ctypes.data, cal.ctypes.data, 1,
                                            C.c_void_p(stream or 0), hits.ctypes.data),
               allow=(UNC_ERR_OVERFLOW,) if allow_overflow else ())
        return hits

    def begin_batch(self, raw, offsets_u64, calib, on_device=False, stream=None):
        """unc_map_batch_begin: stage the reads and launch the kernels (raw: a host int16 array, or with on_device the integer device address
        of the samples); returns at once.  end_batch() waits and returns HIT[n_reads].  One batch per mapper at a time."""
        off = np.ascontiguousarray(offsets_u64, dtype=np.uint64)
        cal = np.ascontiguousarray(calib, dtype=CALIB)
        self._pending_n = off.size - 1
        if on_device:
            ptr = C.c_void_p(raw)
        else:
            self._pending_raw = np.ascontiguousarray(raw, dtype=np.int16)      # (must outlive the call: the copy to the device is asynchronous)
            ptr = C.c_void_p(self._pending_raw.ctypes.data)
        _check(self.L, self.L.unc_map_batch_begin(self.h, self._pending_n, ptr, off.ctypes.data, cal.ctypes.data, 1 if on_device else 0,
                                                  C.c_void_p(stream or 0)))

    def end_batch(self, allow_overflow=False):
        hits = np.zeros(self._pending_n, dtype=HIT)
        _check(self.L, self.L.unc_map_batch_end(self.h, hits.ctypes.data), allow=(UNC_ERR_OVERFLOW,) if allow_overflow else ())
        self._pending_raw = None
        return hits

    def last_timing(self):
        a, b = C.c_float(), C.c_float()
        self.L.unc_mapper_last_timing(self.h, C.byref(a), C.byref(b))
        return a.value, b.value

    def last_window(self):
        """(start, end) of the last batch's k_map in ms on the process-wide time axis (unc_mapper_last_window)"""
        a, b = C.c_double(), C.c_double()
        _check(self.L, self.L.unc_mapper_last_window(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def last_remap(self):
        n, ms = C.c_uint32(), C.c_float()
        self.L.unc_mapper_last_remap(self.h, C.byref(n), C.byref(ms))
        return int(n.value), float(ms.value)

    def set_read_order(self, order):
        """ORDER_INDEPENDENT (default: every read as a fresh Mapper maps it) or ORDER_T1 (`uncalled map -t 1`: one Mapper, reads in
        the order given, sources_added_ carried from read to read and batch to batch); see include/uncalled_hip.h"""
        _check(self.L, self.L.unc_mapper_set_read_order(self.h, int(order)))

    def last_carry_over(self):
        """ORDER_T1: (reads of the last batch mapped again because their predecessor left flags set, rounds, ms)"""
        n, r, ms = C.c_uint32(), C.c_uint32(), C.c_float()
        self.L.unc_mapper_last_carry_over(self.h, C.byref(n), C.byref(r), C.byref(ms))
        return int(n.value), int(r.value), float(ms.value)

    def geometry(self):
        out = np.zeros(5, dtype=np.uint32)
        self.L.unc_mapper_geometry(self.h, out.ctypes.data)
        return dict(zip(("n_waves", "n_slots", "slice_events", "pool_chunks", "max_clusters"), (int(x) for x in out)))

    def sched_parts(self):
        """Pairs of scheduler rings (one per XCD where the slots divide; 0: no time slicing)."""
        self.L.unc_mapper_sched_parts.restype = C.c_uint32
        self.L.unc_mapper_sched_parts.argtypes = [C.c_void_p]
        return int(self.L.unc_mapper_sched_parts(self.h))

    def pool_usage(self):
        """Seed-cluster node pool: chunks (192 KB each) held now, high-water mark of chunks out at once in the last batch / ever,
        times the library resized it (cut to four times the high-water mark when it holds more than eight times that, doubled when found dry; include/uncalled_hip.h)."""
        if not hasattr(self.L, "unc_mapper_pool_usage"):
            return None
        out = np.zeros(4, dtype=np.uint32)
        _check(self.L, self.L.unc_mapper_pool_usage(self.h, out.ctypes.data))
        d = dict(zip(("chunks", "high_water_last_batch", "high_water_ever", "resizes"), (int(x) for x in out)))
        d["gb"] = round(d["chunks"] * 192 * 1024 / 1e9, 2)
        return d

    def kernel_info(self):
        """Register / scratch / LDS figures of the k_map instantiation this mapper launches, read off the code object."""
        out = np.zeros(6, dtype=np.uint32)
        _check(self.L, self.L.unc_mapper_kernel_info(self.h, out.ctypes.data))
        d = dict(zip(("vgprs", "scratch_bytes_per_lane", "lds_bytes", "max_threads", "waves_per_cu", "rows32"), (int(x) for x in out)))
        d["rows32"] = bool(d["rows32"])
        return d

    def set_profile(self, on=True):
        self.L.unc_mapper_set_profile(self.h, 1 if on else 0)

    def last_wave_busy(self):
        return float(self.L.unc_mapper_last_wave_busy(self.h))

    def last_phase_cycles(self):
        out = np.zeros(12, dtype=np.uint64)
        self.L.unc_mapper_last_phase_cycles(self.h, out.ctypes.data)
        return dict(zip(("probs", "extend_rest", "sort", "walk", "sources", "sa", "add_seed", "rest", "e1_parents", "e2_fm", "e3_slots", "e4_children"), out.tolist()))

    def last_read_cycles(self, n_reads):
        """Per read of the last batch: [n_reads, 14] -- twelve phase counters, residence ticks, XCC_ID | HW_ID << 8 (profiling on)."""
        out = np.zeros((int(n_reads), 14), dtype=np.uint64)
        _check(self.L, self.L.unc_mapper_last_read_cycles(self.h, int(n_reads), out.ctypes.data))
        return out

    def detect_events(self, raw_i16, offsets_u64, calib):
        raw = np.ascontiguousarray(raw_i16, dtype=np.int16)
        off = np.ascontiguousarray(offsets_u64, dtype=np.uint64)
        cal = np.ascontiguousarray(calib, dtype=CALIB)
        n = off.size - 1
        means = np.empty(int(off[-1] - off[0]) + 16, dtype=np.float32)
        moff = np.empty(n + 1, dtype=np.uint64)
        info = np.zeros(n, dtype=EVT_INFO)
        _check(self.L, self.L.unc_detect_events(self.h, n, raw.ctypes.data, off.ctypes.data, cal.ctypes.data,
                                                means.ctypes.data, means.size, moff.ctypes.data, info.ctypes.data))
        return means[:int(moff[-1])], moff, info

    def trace(self, raw_i16, calib1, events_per_step=1, max_clusters=1 << 15):
        """Generator over Mapper::map_next steps of one read: (done, paths, clusters, max_map, len_sum, n_lens)."""
        raw = np.ascontiguousarray(raw_i16, dtype=np.int16)
        cal = np.ascontiguousarray(calib1, dtype=CALIB)
        _check(self.L, self.L.unc_trace_begin(self.h, raw.ctypes.data, raw.size, cal.ctypes.data))
        mp = self.params.max_paths
        paths = np.zeros(mp, dtype=PATH)
        clus = np.zeros(max_clusters, dtype=CLUSTER)
        mm = np.zeros(1, dtype=CLUSTER)
        while True:
            done = C.c_int()
            _check(self.L, self.L.unc_trace_step(self.h, events_per_step, C.byref(done)))
            n, nc, nl, ls = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_float()
            _check(self.L, self.L.unc_trace_paths(self.h, paths.ctypes.data, mp, C.byref(n)))
            _check(self.L, self.L.unc_trace_clusters(self.h, clus.ctypes.data, max_clusters, C.byref(nc), mm.ctypes.data,
                                                     C.byref(ls), C.byref(nl)))
            yield bool(done.value), paths[:n.value].copy(), clus[:nc.value].copy(), mm[0].copy(), ls.value, nl.value
            if done.value:
                break

    def trace_finish(self):
        hit = np.zeros(1, dtype=HIT)
        _check(self.L, self.L.unc_trace_finish(self.h, hit.ctypes.data))
        return hit[0]


RT_TAP = np.dtype([("det_t", "<u4"), ("det_total_events", "<u4"), ("det_len_sum", "<f4"), ("norm_n", "<u4"), ("norm_wr", "<u4"),
                   ("prof_n", "<u4"), ("prof_to_mask", "<u4"), ("prof_queued", "<u4"), ("norm_mean", "<f8"), ("norm_varsum", "<f8"),
                   ("prof_mean", "<f8"), ("prof_varsum", "<f8"), ("prof_queue", "<f4", (28,))], align=True)


class Realtime:
    """Chunked path: RealtimePool + one Mapper per channel with MapPoolOrd's deterministic semantics
    (realtime_pool.cpp:74-142,349-358; map_pool_ord.cpp:61-112)."""

    def __init__(self, index, n_channels=512, params=None):
        self.index = index
        self.L = index.L
        self.params = params or default_params(self.L)
        self.n_channels = n_channels
        h = C.c_void_p()
        _check(self.L, self.L.unc_rt_create(index.h, C.byref(self.params), n_channels, C.byref(h)))
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.L.unc_rt_free(self.h)
            self.h = None

    __del__ = close

    def device_bytes(self):
        return self.L.unc_rt_device_bytes(self.h)

    def tap_channel(self, channel):
        """unc_rt_tap_channel: (tap record, ring of 6000 floats) of one channel (parity tests)"""
        tap = np.zeros(1, dtype=RT_TAP)
        ring = np.zeros(6000, dtype=np.float32)
        _check(self.L, self.L.unc_rt_tap_channel(self.h, int(channel), tap.ctypes.data, ring.ctypes.data))
        return tap[0], ring

    def process_chunks(self, chunks, raw_i16=None, raw_ptr=None, stream=None, allow_overflow=False):
        """chunks: RT_CHUNK array (at most one per channel); raw: host int16 array or a device address."""
        ch = np.ascontiguousarray(chunks, dtype=RT_CHUNK)
        res = np.zeros(ch.size, dtype=RT_RESULT)
        if raw_ptr is not None:
            ptr, on_dev = C.c_void_p(raw_ptr), 1
        else:
            raw = np.ascontiguousarray(raw_i16, dtype=np.int16)
            ptr, on_dev = C.c_void_p(raw.ctypes.data), 0
        _check(self.L, self.L.unc_rt_process_chunks(self.h, ch.size, ch.ctypes.data, ptr, on_dev, C.c_void_p(stream or 0),
                                                    res.ctypes.data), allow=(UNC_ERR_OVERFLOW,) if allow_overflow else ())
        return res

    def process_chunks_f32(self, chunks, signal_f32):
        """the same for chunks that hold floats already (what the reference's Chunk keeps): `offset` indexes signal_f32"""
        ch = np.ascontiguousarray(chunks, dtype=RT_CHUNK)
        res = np.zeros(ch.size, dtype=RT_RESULT)
        sig = np.ascontiguousarray(signal_f32, dtype=np.float32)
        _check(self.L, self.L.unc_rt_process_chunks_f32(self.h, ch.size, ch.ctypes.data, C.c_void_p(sig.ctypes.data), 0, None,
                                                        res.ctypes.data))
        return res

    def last_timing(self):
        a, b = C.c_float(), C.c_float()
        self.L.unc_rt_last_timing(self.h, C.byref(a), C.byref(b))
        return a.value, b.value
