"""`-m gpu`: the parity tests proper.  The gfx950 library, called through the C ABI on a real MI355X, against the
oracle restatement on the same seeded inputs, against the committed reference goldens, and -- at the bench's
index scale -- on a synthetic E. coli-sized reference built on the fly."""
import time

import numpy as np
import pytest

from tests import parity_cases as pc
from tests.helpers import assert_hits_equal, oracle_hits
from tools.simulate_reads import CAL_DIGITISATION, CAL_OFFSET, CAL_RANGE, simulate_reads
from uncalled_amd import capi

pytestmark = pytest.mark.gpu


def test_index_tables(hip_lib, oracle_lib, example, goldens):
    pc.case_index_tables(hip_lib, oracle_lib, example, goldens)


def test_fm_primitives(hip_lib, oracle_lib, example, goldens):
    pc.case_fm_primitives(hip_lib, oracle_lib, example, goldens)


@pytest.mark.parametrize("name", pc.FM_REFERENCES)
def test_fm_layer_on_tiny_references(hip_lib, oracle_lib, tmp_path, monkeypatch, name):
    """tests/test_lanesim_parity.py::test_fm_layer_on_tiny_references on the GPU"""
    pc.case_fm_tiny(hip_lib, oracle_lib, tmp_path, monkeypatch, name)


def test_match_probs_over_the_level_range(hip_lib, oracle_lib, example):
    pc.case_match_probs_levels(hip_lib, oracle_lib, example)


def test_events_and_normaliser(hip_lib, oracle_lib, example, goldens):
    pc.case_events_and_normaliser(hip_lib, oracle_lib, example, goldens)


def test_events_of_the_reads_the_sweep_found_wrong(hip_lib, oracle_lib, example):
    pc.case_events_sweep_reads(hip_lib, oracle_lib, example)


def test_events_edge_cases(hip_lib, oracle_lib, example, goldens):
    pc.case_events_edge_cases(hip_lib, oracle_lib, example, goldens)


def test_example_read_full_path(hip_lib, oracle_lib, example, goldens):
    pc.case_example_read_full_path(hip_lib, oracle_lib, example, goldens)


@pytest.mark.parametrize("max_paths,n_reads", [(10000, 48), (300, 24), (97, 12)])
def test_synthetic_batch(hip_lib, oracle_lib, example, goldens, max_paths, n_reads):
    pc.case_synthetic_batch(hip_lib, oracle_lib, example, goldens, max_paths, n_reads)


@pytest.mark.parametrize("max_paths,n_reads,split", [(97, 24, 7), (130, 32, 20), (200, 48, 1)])
def test_read_order_t1(hip_lib, oracle_lib, example, goldens, max_paths, n_reads, split):
    pc.case_read_order_t1(hip_lib, oracle_lib, example, goldens, max_paths, n_reads, split)


def test_read_order_t1_under_pressure(hip_lib, oracle_lib, example, goldens):
    pc.case_read_order_t1_under_pressure(hip_lib, oracle_lib, example, goldens)


def test_trace_matches_oracle_every_event(hip_lib, oracle_lib, example, goldens):
    pc.case_trace_matches_oracle_every_event(hip_lib, oracle_lib, example, goldens)


@pytest.mark.parametrize("n_channels,n_reads,max_chunks,long_read", [(1, 31, None, False), (3, 31, None, False), (2, 8, 2, False),
                                                                   (2, 6, None, True)])
def test_chunked_realtime_path(hip_lib, oracle_lib, example, goldens, n_channels, n_reads, max_chunks, long_read):
    pc.case_chunked_realtime_path(hip_lib, oracle_lib, example, goldens, n_channels, n_reads, max_chunks, long_read)


@pytest.mark.parametrize("n_channels", [2, 3])
def test_chunked_rejected_call_leaves_no_trace(hip_lib, oracle_lib, example, goldens, n_channels):
    pc.case_chunked_rejected_call_leaves_no_trace(hip_lib, oracle_lib, example, goldens, n_channels)


def test_chunked_ignored_chunks(hip_lib, oracle_lib, example, goldens):
    pc.case_chunked_ignored_chunks(hip_lib, oracle_lib, example, goldens)


def test_cluster_overflow_remap(hip_lib, oracle_lib, example, goldens):
    pc.case_cluster_overflow_remap(hip_lib, oracle_lib, example, goldens)


@pytest.mark.parametrize("shift", [4, 8])
def test_narrow_buckets(hip_lib, oracle_lib, example, goldens, monkeypatch, shift):
    pc.case_narrow_buckets(hip_lib, oracle_lib, example, goldens, monkeypatch, shift)


def test_loud_overflows(hip_lib, oracle_lib, example, goldens):
    pc.case_loud_overflows(hip_lib, oracle_lib, example, goldens)


def test_unsorted_stream_past_one_block(hip_lib, oracle_lib, tmp_path):
    pc.case_unsorted_stream_past_one_block(hip_lib, oracle_lib, tmp_path)


def test_chunked_flags_carry_over(hip_lib, oracle_lib, tmp_path):
    pc.case_chunked_flags_carry_over(hip_lib, oracle_lib, tmp_path)


def test_chunked_stage_tap(hip_lib, oracle_lib, example, goldens):
    pc.case_chunked_stage_tap(hip_lib, oracle_lib, example, goldens)


def test_chunked_stage_tap_37_sample_chunks(hip_lib, oracle_lib, example, goldens):
    """the same taps when a chunk ends at every phase of the detector's ring: two reads of 3000 samples in chunks of 37"""
    pc.case_chunked_stage_tap(hip_lib, oracle_lib, example, goldens, n_reads=2, chunk_len=37, cut=3000)


def test_chunked_variants(hip_lib, oracle_lib, example, goldens):
    pc.case_chunked_variants(hip_lib, oracle_lib, example, goldens)


def test_parameter_variants(hip_lib, oracle_lib, example, goldens):
    pc.case_parameter_variants(hip_lib, oracle_lib, example, goldens)


def test_batch_in_two_halves(hip_lib, oracle_lib, example, goldens):
    pc.case_batch_in_two_halves(hip_lib, oracle_lib, example, goldens, n_reads=24)


def test_same_row_two_kmers_walked_again_on_wide_keys(hip_lib, oracle_lib, tmp_path):
    pc.case_same_row_two_kmers(hip_lib, oracle_lib, tmp_path)


def test_merge_walk_mid_reference(hip_lib, oracle_lib, tmp_path):
    pc.case_mid_reference(hip_lib, oracle_lib, tmp_path)


def test_wide_sort_keys(hip_lib, oracle_lib, example, goldens, monkeypatch):
    pc.case_wide_sort_keys(hip_lib, oracle_lib, example, goldens, monkeypatch)


@pytest.fixture(scope="module")
def ecoli(tmp_path_factory):
    """SURVEY 8(d) `ecoli_syn`: 4 641 652 bp i.i.d. genome, seed 1, index in BWA format (uncalled_amd/build_index.py)."""
    from uncalled_amd.build_index import build_from_codes, synthetic_genome
    d = tmp_path_factory.mktemp("ecoli")
    names, lens, codes = synthetic_genome(1, 4641652, seed=1)
    prefix = d / "ecoli_syn"
    build_from_codes(prefix, names, [""] * len(names), lens, codes)
    from uncalled_amd.index_params import parameterize
    parameterize(capi.Index(prefix), prefix)          # `uncalled index`: this reference's own .uncl
    return dict(prefix=prefix, codes=codes, lens=lens)


def test_ecoli_scale_batch(hip_lib, oracle_lib, ecoli):
    """4 096 full-length (3600-base, about 32 k-sample) reads, mapped + off-target, against the oracle on all host threads: PAF,
    winning cluster, event counts and work counters bit-exact.  (Rounds 1-5: 192 reads -- a suite that could not see a defect that
    strikes one read in seven thousand, round-5 review; at 4 096 reads of the headline workload a 1e-3 defect shows with 98 %.)"""
    from tests.helpers import oracle_hits_threads
    from tools.simulate_reads_torch import simulate_reads_torch
    n = 4096
    sim = simulate_reads_torch(ecoli["codes"], ecoli["lens"], n, seed=42, device="cuda:0")
    raw = sim["signal"].cpu().numpy()
    off = sim["offsets"]
    cal = capi.make_calib(n, CAL_RANGE, CAL_OFFSET, CAL_DIGITISATION)
    ix = capi.Index(ecoli["prefix"], lib=hip_lib)
    m = capi.Mapper(ix)
    t0 = time.time()
    hits = m.map_batch(raw, off, cal)
    t_gpu = time.time() - t0
    oix = oracle_lib.Index(ecoli["prefix"])
    want, t_cpu, redone = oracle_hits_threads(oix, raw, off, cal, hits)
    assert_hits_equal(hits, want, "ecoli")
    assert redone <= 4            # (reads that follow a read with sources_added_ left set on their oracle thread: a handful in 50 000)
    mapped = int(hits["mapped"].sum())
    assert mapped >= 0.7 * n
    ok = 0
    for i in np.flatnonzero(hits["mapped"]):
        if sim["contig"][i] >= 0 and bool(hits["fwd"][i]) == (sim["strand"][i] == 0) and \
                sim["pos"][i] - 100 <= hits["rf_st"][i] <= sim["pos"][i] + 3700:
            ok += 1
    assert ok >= 0.95 * mapped
    print(f"ecoli batch: {n} reads, {mapped} mapped, gpu {t_gpu:.2f}s, oracle (all host threads) {t_cpu:.2f}s, {redone} mapped again by a fresh oracle Mapper")


def test_batch_order_and_slot_independence(hip_lib, oracle_lib, example, goldens):
    """A read's result does not depend on which slot / in which order it is processed (no state leaks across
    reads): map the golden batch reversed and with a single slot."""
    n = 32
    off = goldens["sim_offsets"]
    reads = [goldens["sim_signal"][int(off[i]):int(off[i + 1])] for i in range(n)]
    cal = capi.make_calib(n, CAL_RANGE, CAL_OFFSET, CAL_DIGITISATION)
    ix = capi.Index(example["prefix"], lib=hip_lib)

    def run(order, n_slots):
        raw = np.concatenate([reads[i] for i in order])
        o = np.concatenate(([0], np.cumsum([len(reads[i]) for i in order]))).astype(np.uint64)
        h = capi.Mapper(ix, n_slots=n_slots).map_batch(raw, o, cal)
        out = np.zeros_like(h)
        out[list(order)] = h
        return out
    a = run(range(n), 0)
    b = run(range(n - 1, -1, -1), 1)
    for f in ("mapped", "rd_st", "rd_en", "rf_st", "rf_en", "matches", "event_i", "n_nbr", "n_sa", "n_lf"):
        assert np.array_equal(a[f], b[f]), f


@pytest.fixture(scope="module")
def chr20(tmp_path_factory):
    """SURVEY 8(d) `chr20_syn`: 64 444 167 bp, seed 2, 30 % of the length in N-runs (filled with seeded random bases and
    recorded in .amb), BWA-format index with the suffix array built on the GPU (uncalled_amd/build_index.py)."""
    from uncalled_amd.build_index import build_from_codes, masked_synthetic_genome
    d = tmp_path_factory.mktemp("chr20")
    names, lens, codes, holes, n_ambs = masked_synthetic_genome(1, 64444167, seed=2, name="chr20_syn")
    prefix = d / "chr20_syn"
    build_from_codes(prefix, names, [""] * len(names), lens, codes, holes, n_ambs, sa_device="cuda")
    from uncalled_amd.index_params import parameterize
    parameterize(capi.Index(prefix), prefix)
    return dict(prefix=prefix, codes=codes, lens=lens)


def test_chr20_scale_batch(hip_lib, oracle_lib, chr20):
    """Config 3's index scale (seq_len 128.9 M: 64 MB of FM blocks + 1 GB dense SA, beyond any L2): 1 024 reads against
    the oracle on all host threads, bit-exact (rounds 1-5: 96)."""
    from tests.helpers import oracle_hits_threads
    from tools.simulate_reads_torch import simulate_reads_torch
    n = 1024
    sim = simulate_reads_torch(chr20["codes"], chr20["lens"], n, seed=43, device="cuda:0")
    raw = sim["signal"].cpu().numpy()
    off = sim["offsets"]
    cal = capi.make_calib(n, CAL_RANGE, CAL_OFFSET, CAL_DIGITISATION)
    ix = capi.Index(chr20["prefix"], lib=hip_lib)
    assert ix.size == 2 * 64444167
    m = capi.Mapper(ix)
    hits = m.map_batch(raw, off, cal)
    oix = oracle_lib.Index(chr20["prefix"])
    want, _secs, redone = oracle_hits_threads(oix, raw, off, cal, hits)
    assert_hits_equal(hits, want, "chr20")
    assert redone <= 2 and int(hits["mapped"].sum()) >= 0.5 * n


@pytest.mark.parametrize("max_paths,slice_events,n_slots,n_waves", [(10000, 37, 5, 2), (300, 11, 3, 1), (10000, 200, 9, 4)])
def test_sliced_scheduler(hip_lib, oracle_lib, example, goldens, max_paths, slice_events, n_slots, n_waves):
    pc.case_sliced_scheduler(hip_lib, oracle_lib, example, goldens, max_paths, slice_events, n_slots, n_waves)


def test_scheduler_rings_per_xcd(hip_lib, oracle_lib, example, goldens):
    """On the GPU the eight wavefronts really sit on eight XCDs: every share's rings are in use, and parked reads are resumed out of an L2
    that nobody wrote back or invalidated in between."""
    assert pc.case_scheduler_rings_per_xcd(hip_lib, oracle_lib, example, goldens, n_reads=24) == 8


@pytest.mark.parametrize("pool_chunks,n_waves", [(3, 2), (1, 1)])
def test_cluster_pool_pressure(hip_lib, oracle_lib, example, goldens, pool_chunks, n_waves):
    pc.case_cluster_pool_pressure(hip_lib, oracle_lib, example, goldens, pool_chunks, n_waves)


def test_creation_sizes(hip_lib, example, monkeypatch):
    """device_bytes of the three index loads, of three mappers and of a realtime mapper whose sizes are all named, and the mappers'
    geometry: the constants of parity_cases.py, the same under the emulator and on the GPU."""
    pc.case_creation_sizes(hip_lib, example, monkeypatch)


def test_big_forests(hip_lib, oracle_lib, example, goldens, tmp_path, monkeypatch):
    pc.case_big_forests(hip_lib, oracle_lib, example, goldens, tmp_path, monkeypatch)


@pytest.mark.parametrize("team", [8, 4, 2, 1])
def test_chunked_mid_reference_team_sort(hip_lib, oracle_lib, tmp_path, monkeypatch, team):
    monkeypatch.setenv("UNC_RT_TEAM", str(team))
    pc.case_chunked_mid_reference(hip_lib, oracle_lib, tmp_path, n=4, cut=8000)


@pytest.mark.parametrize("team", [8, 1])
def test_chunked_pool_chunks_go_back(hip_lib, oracle_lib, example, goldens, monkeypatch, team):
    """tests/test_lanesim_parity.py: a pool of two chunks, twelve reads in a row on one channel"""
    monkeypatch.setenv("UNC_RT_TEAM", str(team))
    monkeypatch.setenv("UNC_RT_POOL_CHUNKS", "2")
    pc.case_chunked_realtime_path(hip_lib, oracle_lib, example, goldens, 1, 12, None)


@pytest.mark.parametrize("team", [8, 2])
def test_team_round_that_fills_the_buffer_exactly(hip_lib, team):
    from pathlib import Path
    from tests.test_lanesim_parity import _fuzz_round
    _fuzz_round(Path(__file__).resolve().parents[1] / "uncalled_amd" / "libuncalled_hip.so", 9512, "rt", team)


# ---- calibrations other than the simulators' (tests/helpers.py REGIMES)

def test_calibration_through_event_means(hip_lib, oracle_lib, example):
    pc.case_calibration_through_event_means(hip_lib, oracle_lib, example)


def test_event_mean_bounds(hip_lib, oracle_lib, example):
    pc.case_event_mean_bounds(hip_lib, oracle_lib, example)


def test_zero_pa_windows(hip_lib, oracle_lib, example):
    pc.case_zero_pa_windows(hip_lib, oracle_lib, example)


def test_per_read_calibration_batch(hip_lib, oracle_lib, example, goldens):
    import torch
    held = []

    def to_device(raw):
        t = torch.from_numpy(np.ascontiguousarray(raw)).to("cuda:0")
        torch.cuda.synchronize()
        held.append(t)
        return t.data_ptr()
    share = pc.case_per_read_calibration_batch(hip_lib, oracle_lib, example, goldens, n_reads=40, device=to_device)
    print("per-read calibration batch, mapped / reads per regime:", share)


def test_trace_under_another_calibration(hip_lib, oracle_lib, example, goldens):
    pc.case_trace_under_another_calibration(hip_lib, oracle_lib, example, goldens)


def test_refused_while_pending(hip_lib, oracle_lib, example, goldens):
    pc.case_refused_while_pending(hip_lib, oracle_lib, example, goldens)


@pytest.mark.parametrize("shuffle,f32", [(False, False), (True, False), (True, True)])
def test_chunked_per_channel_calibration(hip_lib, oracle_lib, example, goldens, shuffle, f32):
    pc.case_chunked_per_channel_calibration(hip_lib, oracle_lib, example, goldens, n_channels=6, reads_per_channel=3, shuffle=shuffle, f32=f32)


def test_chunked_512_channels_per_channel_calibration(hip_lib, oracle_lib, example, goldens, monkeypatch):
    """config 5's width: 512 channels on teams of 8, two reads each, every channel and read under a calibration of its own, rounds
    shuffled and thinned; every read against its channel's oracle Mapper"""
    monkeypatch.setenv("UNC_RT_TEAM", "8")
    mapped, n = pc.case_chunked_per_channel_calibration(hip_lib, oracle_lib, example, goldens, n_channels=512, reads_per_channel=2, shuffle=True)
    print(f"512 channels: {mapped} of {n} reads mapped")


@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("lanes", [2, 3, 64])
def test_rt_event_lanes(hip_lib, oracle_lib, example, goldens, monkeypatch, lanes, f32):
    """k_rt_events with 2, 3 and 64 channels per wavefront: everything in it that depends on the lane, which calls of at most 2048
    chunks never run past lane 0"""
    pc.case_rt_event_lanes(hip_lib, oracle_lib, example, goldens, monkeypatch, lanes, f32)


def test_rt_event_lanes_refused(hip_lib, example, monkeypatch):
    pc.case_rt_event_lanes_refused(hip_lib, example, monkeypatch)


@pytest.mark.parametrize("lanes", [None, 64])
def test_chunked_reads_that_end_early(hip_lib, oracle_lib, example, goldens, monkeypatch, lanes):
    pc.case_chunked_reads_that_end_early(hip_lib, oracle_lib, example, goldens, monkeypatch, lanes)


@pytest.mark.parametrize("wide,chunk_len,f32", pc.ZERO_PA_CHUNKED)
def test_chunked_zero_pa_windows(hip_lib, oracle_lib, example, wide, chunk_len, f32):
    pc.case_chunked_zero_pa_windows(hip_lib, oracle_lib, example, wide, chunk_len, f32)


def test_chunked_samples_that_are_no_numbers(hip_lib, oracle_lib, example, goldens):
    pc.case_chunked_samples_that_are_no_numbers(hip_lib, oracle_lib, example, goldens)


def test_chunked_ring_wraps_then_short_reads(hip_lib, oracle_lib, example, goldens):
    pc.case_chunked_ring_wraps_then_short_reads(hip_lib, oracle_lib, example, goldens)


def test_staging_buffers_reused_after_begin(hip_lib, oracle_lib, example, goldens):
    """`offsets` and `calib` are copied by unc_map_batch_begin (include/uncalled_hip.h): in page-locked memory (unc_host_alloc), begun on
    a stream with another mapper's batch queued ahead, and overwritten -- other calibrations, read boundaries moved by a few samples --
    as soon as _begin returns, the batch still maps what it was given.  (The overwriting values are valid: a copy that ran late would
    give wrong hits, never an access out of bounds.)"""
    import ctypes as C
    import torch
    from tests.helpers import assert_hits_equal
    raw, off, cal, _ = pc.per_read_regime_batch(goldens, 24, seed=23)
    n = off.size - 1
    want = oracle_hits(oracle_lib.Index(example["prefix"]), raw, off, cal, fresh_mapper_per_read=True)
    ix = capi.Index(example["prefix"], lib=hip_lib)
    go = goldens["sim_offsets"]
    big_raw = np.tile(goldens["sim_signal"][:int(go[-1])], 4)
    big_off = np.concatenate([go[:-1] + k * go[-1] for k in range(4)] + [[4 * go[-1]]]).astype(np.uint64)
    blocker = capi.Mapper(ix, n_slots=4, n_waves=4)
    m = capi.Mapper(ix, n_slots=8)
    nb_off, nb_cal = (n + 1) * 8, n * capi.CALIB.itemsize
    buf = hip_lib.unc_host_alloc(nb_off + nb_cal)
    assert buf
    try:
        a = np.ctypeslib.as_array(C.cast(buf, C.POINTER(C.c_uint8)), shape=(nb_off + nb_cal,))
        p_off, p_cal = a[:nb_off].view(np.uint64), a[nb_off:].view(capi.CALIB)
        p_off[:] = off
        p_cal[:] = cal
        moved = off.copy()
        moved[1:-1] = off[1:-1] + np.where(np.arange(1, n) % 2 == 1, 3, -3).astype(np.uint64)     # same first and last offset
        s = torch.cuda.Stream()
        blocker.begin_batch(big_raw, big_off, capi.make_calib(big_off.size - 1, CAL_RANGE, CAL_OFFSET, CAL_DIGITISATION), stream=s.cuda_stream)
        m.begin_batch(raw, p_off, p_cal, stream=s.cuda_stream)
        p_off[:] = moved
        p_cal[:] = np.roll(cal, 1)               # every read another regime
        hits = m.end_batch()
        blocker.end_batch()
        assert_hits_equal(hits, want, "offsets and calib reused after _begin")
    finally:
        torch.cuda.synchronize()
        hip_lib.unc_host_free(buf)


def test_ecoli_scale_per_read_calibration(hip_lib, oracle_lib, ecoli):
    """1 024 E. coli reads, each re-digitised for a calibration regime of its own (neighbours differ), against the oracle on all host
    threads -- which calibrates every read with its own entry (tests/helpers.py oracle_hits_threads)"""
    from tests.helpers import REGIMES, calib_of, oracle_hits_threads, redigitise
    from tools.simulate_reads_torch import simulate_reads_torch
    n = 1024
    sim = simulate_reads_torch(ecoli["codes"], ecoli["lens"], n, seed=44, device="cuda:0")
    raw0 = sim["signal"].cpu().numpy()
    off = sim["offsets"]
    names = list(REGIMES)
    rng = np.random.default_rng(44)
    pick = [0]
    while len(pick) < n:
        k = int(rng.integers(0, len(names)))
        if k != pick[-1]:
            pick.append(k)
    raw = raw0.copy()
    for i, k in enumerate(pick):
        a, b = int(off[i]), int(off[i + 1])
        raw[a:b] = redigitise(raw0[a:b], REGIMES["minion"], REGIMES[names[k]])
    cal = calib_of([REGIMES[names[k]] for k in pick])
    ix = capi.Index(ecoli["prefix"], lib=hip_lib)
    hits = capi.Mapper(ix).map_batch(raw, off, cal)
    want, _secs, redone = oracle_hits_threads(oracle_lib.Index(ecoli["prefix"]), raw, off, cal, hits)
    assert_hits_equal(hits, want, "ecoli, per-read calibration")
    assert redone <= 2
    share = {}
    for j, name in enumerate(names):
        sel = np.array(pick) == j
        share[name] = (int(hits["mapped"][sel].sum()), int(sel.sum()))
        assert share[name][0] >= 0.6 * share[name][1], share
    print("ecoli per-read calibration, mapped / reads per regime:", share)
