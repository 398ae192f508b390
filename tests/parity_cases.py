"""Parity cases shared by the lanesim (CPU emulator, container) and gpu (real MI355X) test modules: the HIP path
-- through the C ABI -- against the oracle restatement and the committed reference goldens."""
from pathlib import Path

import numpy as np
import pytest

from tests.helpers import assert_hits_equal, oracle_hits, to_oracle_params
from tools.simulate_reads import CAL_DIGITISATION, CAL_OFFSET, CAL_RANGE
from uncalled_amd import capi

_cache = {}
GOLDEN_DIR = Path(__file__).resolve().parent / "golden"


def _index(lib, example):
    key = (id(lib), str(example["prefix"]))
    if key not in _cache:
        _cache[key] = capi.Index(example["prefix"], lib=lib)
    return _cache[key]


def case_index_tables(lib, oracle_lib, example, goldens):
    dev_index = _index(lib, example)
    oix = oracle_lib.Index(example["prefix"])
    assert np.array_equal(dev_index.kmer_ranges(), oix.kmer_ranges())
    assert np.array_equal(dev_index.thresholds(), oix.thresholds())
    for a, b in zip(dev_index.model_tables(), oracle_lib.model_tables()):
        assert np.array_equal(np.asarray(a), np.asarray(b))


def case_fm_primitives(lib, oracle_lib, example, goldens):
    dev_index = _index(lib, example)
    oix = oracle_lib.Index(example["prefix"])
    rng = np.random.default_rng(1)
    kr = oix.kmer_ranges()
    s, e, b = [], [], []
    for k in rng.integers(0, 1024, 300):
        if kr[k, 0] <= kr[k, 1]:
            lo = int(rng.integers(kr[k, 0], kr[k, 1] + 1))
            hi = int(rng.integers(lo, kr[k, 1] + 1))
            s.append(lo); e.append(hi); b.append(int(rng.integers(0, 4)))
    # edge rows: first row, the sentinel row's neighbours, last row
    for row in (1, 2, int(oix.size) - 1, int(oix.size)):
        s.append(row); e.append(row); b.append(int(rng.integers(0, 4)))
    os_, oe = dev_index.get_neighbor(s, e, b)
    for x, y, z, p, q in zip(s, e, b, os_, oe):
        assert oix.get_neighbor(x, y, z) == (int(p), int(q))
    rows = np.concatenate((rng.integers(0, oix.size + 1, 400), [0, 1, oix.size]))
    assert np.array_equal(dev_index.sa(rows), np.array([oix.sa(int(r)) for r in rows], dtype=np.uint64))


def case_events_and_normaliser(lib, oracle_lib, example, goldens):
    dev_index = _index(lib, example)
    m = capi.Mapper(dev_index, n_slots=1)
    raw = example["signal"]
    off = np.array([0, raw.size], dtype=np.uint64)
    cal = capi.make_calib(1, example["range"], example["offset"], example["digitisation"])
    means, moff, info = m.detect_events(raw, off, cal)
    assert np.array_equal(means, goldens["ex_events"]["mean"])          # north star: 1e-5; achieved: bit-exact
    assert info["total_events"][0] == int(goldens["ex_total_events"])
    assert np.float32(info["len_sum"][0] / info["total_events"][0]) == goldens["ex_mean_event_len"]
    assert info["scale"][0] == goldens["ex_scale"] and info["shift"][0] == goldens["ex_shift"]
    lv = goldens["ex_levels"]
    assert np.array_equal(dev_index.match_probs(lv[:64]), goldens["ex_probs"])


def case_radix_sort(lib, big=False):
    rng = np.random.default_rng(1)
    sizes = [(1, 64), (63, 8), (64, 16), (2048, 24), (2049, 64), (5000, 62), (70001, 40)] + ([(3_000_001, 63), (1 << 22, 33)] if big else [(300000, 33)])
    for n, bits in sizes:
        keys = rng.integers(0, 2 ** min(bits, 63), size=n, dtype=np.uint64)
        if bits == 64:
            keys = keys * np.uint64(2) + rng.integers(0, 2, size=n, dtype=np.uint64)
        if n > 100:
            keys[::7] = keys[3]          # ties: a seventh of the keys are equal
        want = np.argsort(keys, kind="stable").astype(np.uint64)
        sk, perm = capi.sort_pairs(keys, None, bits, lib=lib)
        assert np.array_equal(perm, want) and np.array_equal(sk, keys[want]), (n, bits)
        vals = rng.integers(0, 2 ** 63, size=n, dtype=np.uint64)
        sk2, sv = capi.sort_pairs(keys, vals, bits, lib=lib)
        assert np.array_equal(sk2, sk) and np.array_equal(sv, vals[want]), (n, bits)
    case_radix_sort_edges(lib)


def case_events_sweep_reads(lib, oracle_lib, example):
    """Reads the round-5 parity sweeps (10 240 reads each of the chr20 and GRCh38 bench batches against the reference's object code,
    tests/dev/parity_sweep.py) found the device WRONG on: one event too many, because the t-statistic's square root was hipcc's
    __fsqrt_rn = the bare v_sqrt_f32 (1 ulp) and not the correctly rounded sqrtss of the reference (event_detector.cpp:218).  One read
    in seven thousand; the emulator (sqrtf on the host) never saw it.  The raw signals are committed (tests/golden/sweep_reads_r05.npz,
    dumped on the GPU box by tests/dev/dump_reads.py); every kept event mean and both counters must be the oracle's, at every alignment
    of the read inside its batch.  (The oracle's detector is pinned on the reference's own: tests/test_oracle.py.)"""
    d = np.load(GOLDEN_DIR / "sweep_reads_r05.npz")
    dev_index = _index(lib, example)
    m = capi.Mapper(dev_index, n_slots=4)
    for r in (37043, 66882, 61770):
        raw = d[f"raw_{r}"]
        ev, mel, tot = oracle_lib.detect_events(oracle_lib.calibrate(raw, CAL_RANGE, CAL_OFFSET, CAL_DIGITISATION))[:3]
        for pad in (0, 1, int(8 - int(d[f"offmod_{r}"])) % 8 + 8):
            full = np.concatenate((np.full(pad, 500, np.int16), raw))
            off = np.array([0, pad, pad + raw.size], dtype=np.uint64) if pad else np.array([0, raw.size], dtype=np.uint64)
            means, moff, info = m.detect_events(full, off, capi.make_calib(off.size - 1, CAL_RANGE, CAL_OFFSET, CAL_DIGITISATION))
            k = off.size - 2
            assert info["n_events"][k] == len(ev) and info["total_events"][k] == tot, (r, pad, int(info["n_events"][k]), len(ev))
            assert np.array_equal(means[int(moff[k]):int(moff[k + 1])], ev["mean"].astype(np.float32)), (r, pad)
            assert np.float32(info["len_sum"][k] / info["total_events"][k]) == np.float32(mel), (r, pad)


def case_events_edge_cases(lib, oracle_lib, example, goldens):
    """empty read, reads shorter than the detector windows, a flat (zero-variance) read, negative samples."""
    dev_index = _index(lib, example)
    po = oracle_lib
    rng = np.random.default_rng(5)
    reads = [np.zeros(0, np.int16), np.array([500], np.int16), rng.integers(300, 700, 12).astype(np.int16),
             np.full(400, 512, np.int16), rng.integers(-200, 900, 700).astype(np.int16),
             np.repeat(rng.integers(350, 650, 60), 9).astype(np.int16)]
    # k_events takes 8 samples per step from the first 16-byte boundary past sample 16 on: every head / tail length and
    # every alignment of a read inside the batch (step signals, so that events fall into heads and tails as well)
    for ln in list(range(13, 42)) + [63, 64, 65, 127, 129, 1000, 1003]:
        reads.append(np.repeat(rng.integers(330, 680, ln // 5 + 1), 5)[:ln].astype(np.int16) + rng.integers(-6, 7, ln).astype(np.int16))
    raw = np.concatenate(reads)
    off = np.concatenate(([0], np.cumsum([len(r) for r in reads]))).astype(np.uint64)
    cal = capi.make_calib(len(reads), CAL_RANGE, CAL_OFFSET, CAL_DIGITISATION)
    m = capi.Mapper(dev_index, n_slots=1)
    means, moff, info = m.detect_events(raw, off, cal)
    for i, r in enumerate(reads):
        ev, mel, tot = po.detect_events(po.calibrate(r, CAL_RANGE, CAL_OFFSET, CAL_DIGITISATION))
        assert info["n_events"][i] == len(ev) and info["total_events"][i] == tot, i
        assert np.array_equal(means[int(moff[i]):int(moff[i + 1])], ev["mean"]), i
        if len(ev):
            lv, sc, sh = po.normalize(ev["mean"])
            assert (np.float32(sc) == info["scale"][i] or (np.isnan(sc) and np.isnan(info["scale"][i]))), i
            assert (np.float32(sh) == info["shift"][i] or (np.isnan(sh) and np.isnan(info["shift"][i]))), i


def case_example_read_full_path(lib, oracle_lib, example, goldens):
    dev_index = _index(lib, example)
    m = capi.Mapper(dev_index, n_slots=2)
    raw = example["signal"]
    off = np.array([0, raw.size], dtype=np.uint64)
    cal = capi.make_calib(1, example["range"], example["offset"], example["digitisation"])
    hits = m.map_batch(raw, off, cal)
    oix = oracle_lib.Index(example["prefix"])
    assert_hits_equal(hits, oracle_hits(oix, raw, off, cal), "example")
    assert capi.hit_paf_cols(hits[0], dev_index.seq_names()) == \
        (106, 73, 106, "-", "Escherichia_coli_chromosome:2400000-2410000", 10000, 6938, 6976, 38, 39, 255)


def case_synthetic_batch(lib, oracle_lib, example, goldens, max_paths, n_reads):
    """Batch through the persistent read queue (more reads than slots); small max_paths exercises the buffer
    cut-off semantics of mapper.cpp:480-482,507-509,521-523,544,576,605-624 incl. stale sources_added_ flags."""
    dev_index = _index(lib, example)
    p = capi.default_params(dev_index.L)
    p.max_paths = max_paths
    m = capi.Mapper(dev_index, params=p, n_slots=3)
    off_all = goldens["sim_offsets"]
    raw = goldens["sim_signal"][:int(off_all[n_reads])]
    off = off_all[:n_reads + 1].copy()
    cal = capi.make_calib(n_reads, CAL_RANGE, CAL_OFFSET, CAL_DIGITISATION)
    hits = m.map_batch(raw, off, cal)
    oix = oracle_lib.Index(example["prefix"])
    want = oracle_hits(oix, raw, off, cal, to_oracle_params(p), fresh_mapper_per_read=True)
    assert_hits_equal(hits, want, f"max_paths={max_paths}")
    if max_paths == 10000:
        f = {str(n): j for j, n in enumerate(goldens["hit_fields"])}
        for i in range(n_reads):   # and against the reference's own answers
            for name in ("mapped", "rd_st", "rd_en", "rd_len", "rf_st", "rf_en", "matches", "event_i", "n_nbr", "n_lf"):
                assert int(hits[i][name]) == int(goldens["sim_hits"][i][f[name]]), (i, name)


def case_read_order_t1(lib, oracle_lib, example, goldens, max_paths, n_reads, split):
    """UNC_ORDER_T1 = `uncalled map -t 1`: ONE Mapper maps the reads back to back (the oracle with a shared mapper; pinned against the
    reference's own Mapper in test_oracle.py), sources_added_ travelling from read to read -- within a batch and, here, across the
    two batches the reads are handed over in.  A small max_paths makes nearly every read leave flags behind; the case also checks
    that this matters (the independent order gives different answers on the same reads), so that it cannot pass vacuously."""
    dev_index = _index(lib, example)
    p = capi.default_params(dev_index.L)
    p.max_paths = max_paths
    off_all = goldens["sim_offsets"]
    raw = goldens["sim_signal"][:int(off_all[n_reads])]
    off = off_all[:n_reads + 1].copy()
    cal = capi.make_calib(n_reads, CAL_RANGE, CAL_OFFSET, CAL_DIGITISATION)
    oix = oracle_lib.Index(example["prefix"])
    want = oracle_hits(oix, raw, off, cal, to_oracle_params(p), fresh_mapper_per_read=False)
    indep = oracle_hits(oix, raw, off, cal, to_oracle_params(p), fresh_mapper_per_read=True)
    differ = [i for i in range(n_reads) if any(int(want[i][f]) != int(indep[i][f]) for f in ("event_i", "n_nbr", "n_sa", "mapped", "rf_st"))]
    assert differ, "the carry-over changes nothing on these reads: the case proves nothing"
    m = capi.Mapper(dev_index, params=p, n_slots=3)
    m.set_read_order(capi.ORDER_T1)
    a = m.map_batch(raw[:int(off[split])], off[:split + 1].copy(), cal[:split])
    n_a = m.last_carry_over()[0]
    b_off = (off[split:] - off[split]).astype(np.uint64)
    b = m.map_batch(raw[int(off[split]):], b_off, cal[split:])
    n_b = m.last_carry_over()[0]
    assert_hits_equal(np.concatenate([a, b]), want, f"-t 1 order, max_paths={max_paths}")
    assert n_a + n_b > 0
    # a new run starts clear: the first read again as a fresh Mapper maps it
    m.set_read_order(capi.ORDER_T1)
    again = m.map_batch(raw[:int(off[1])], off[:2].copy(), cal[:1])
    assert_hits_equal(again, indep[:1], "first read of a new run")
    # ... and the default order is untouched by all this
    m.set_read_order(capi.ORDER_INDEPENDENT)
    assert_hits_equal(m.map_batch(raw, off, cal), indep, "independent order")


def case_read_order_t1_under_pressure(lib, oracle_lib, example, goldens, n_reads=6):
    """UNC_ORDER_T1 with a node pool of ONE chunk and an allowance of four nodes per read: reads overflow in the first pass AND when they
    are mapped again inside a carry-over round, so the overflow handling runs on the re-mapped reads of a `-t 1` round (its `subset`
    form, which neither case_read_order_t1 -- a roomy pool -- nor case_cluster_pool_pressure -- the independent order -- reaches).  One
    batch, every field against the oracle with a shared mapper; both premises are checked."""
    dev_index = _index(lib, example)
    p = capi.default_params(dev_index.L)
    p.max_paths = 97
    off_all = goldens["sim_offsets"]
    raw = goldens["sim_signal"][:int(off_all[n_reads])]
    off = off_all[:n_reads + 1].copy()
    cal = capi.make_calib(n_reads, CAL_RANGE, CAL_OFFSET, CAL_DIGITISATION)
    want = oracle_hits(oracle_lib.Index(example["prefix"]), raw, off, cal, to_oracle_params(p), fresh_mapper_per_read=False)
    m = capi.Mapper(dev_index, params=p, n_slots=3, n_waves=3, pool_chunks=1, max_clusters=16)
    m.set_read_order(capi.ORDER_T1)
    hits = m.map_batch(raw, off, cal)
    assert_hits_equal(hits, want, "-t 1 order under pool pressure")
    assert m.last_remap()[0] > 0 and m.last_carry_over()[0] > 0, (m.last_remap(), m.last_carry_over())


def case_trace_matches_oracle_every_event(lib, oracle_lib, example, goldens, dev_index=None, raw=None, cal=None):
    """Path buffer (order, ranges, k-mers, prob-sum windows, flags) and the seed-cluster set after every map_next."""
    dev_index = dev_index or _index(lib, example)
    if raw is None:
        raw = example["signal"][:6000]
        cal = (example["range"], example["offset"], example["digitisation"])
    m = capi.Mapper(dev_index, n_slots=1)
    oix = oracle_lib.Index(example["prefix"])
    om = oracle_lib.Mapper(oix)
    sig = oracle_lib.calibrate(raw, *cal)
    cal = capi.make_calib(1, *cal)
    steps = 0
    for (dd, dpaths, dclus, dmm, dls, dnl), (od, oe, opaths, oclus, omm, ols, onl) in zip(m.trace(raw, cal), om.trace(sig)):
        assert dd == od, steps
        v = opaths["length"] > 0          # the device list holds only valid parents, in the same order
        ov = opaths[v]
        assert len(dpaths) == len(ov), steps
        for f in ("fm_start", "fm_end", "kmer", "length", "event_moves", "seed_prob", "consec_stays", "sa_checked"):
            assert np.array_equal(dpaths[f], ov[f]), (steps, f)
        for j in range(len(ov)):
            L = int(ov["length"][j])
            assert np.array_equal(dpaths["prob_sums"][j][:L + 1], ov["prob_sums"][j][:L + 1]), (steps, j)
        assert np.array_equal(dclus, oclus), steps
        assert dls == ols and dnl == onl, steps
        if omm["total_len"]:
            assert dmm == omm, steps
        steps += 1
    assert steps > 100
    dh, oh = m.trace_finish(), om.trace_finish()
    assert_hits_equal([dh], [oh], "trace")


# Parameter sets away from the reference's defaults (mapper.cpp:29-40, event_detector.cpp:17-26, seed_tracker.cpp:28-32): each
# moves a decision the default run hardly ever takes the other way.  tests/test_oracle.py pins the oracle against the live
# reference on every one of them; the device is compared with the oracle.
PARAM_VARIANTS = [
    dict(max_rep_copy=5, min_rep_len=12),                       # repeat seeds: fewer copies, only after 12 moves (mapper.cpp:858-861)
    dict(max_consec_stay=3, max_stay_frac=0.25),                # stay children cut earlier (:470-483), stricter seed validity (:852-854)
    dict(min_seed_prob=-3.2),                                   # fewer seed-valid paths
    dict(max_events=350),                                       # reads that run out of events (:381-405)
    dict(min_map_len=15, min_mean_conf=3.0, min_top_conf=1.2),  # earlier, weaker success (seed_tracker.cpp:129-143)
    dict(threshold1=1.7, threshold2=8.0, peak_height=0.35, min_mean=55.0, max_mean=130.0),   # another segmentation, events dropped by mean
    dict(max_paths=150, max_rep_copy=64, max_consec_stay=12),   # the max_paths cut-off with long stays and the largest repeat copy
]


def variant_params(base, overrides):
    for k, v in overrides.items():
        setattr(base, k, v)
    return base


def case_parameter_variants(lib, oracle_lib, example, goldens, n=6):
    dev_index = _index(lib, example)
    oix = oracle_lib.Index(example["prefix"])
    off = goldens["sim_offsets"][:n + 1].copy()
    raw = goldens["sim_signal"][:int(off[n])]
    cal = capi.make_calib(n, CAL_RANGE, CAL_OFFSET, CAL_DIGITISATION)
    for ov in PARAM_VARIANTS:
        p = variant_params(capi.default_params(lib), ov)
        hits = capi.Mapper(dev_index, params=p, n_slots=3).map_batch(raw, off, cal)
        want = oracle_hits(oix, raw, off, cal, to_oracle_params(p), fresh_mapper_per_read=True)
        assert_hits_equal(hits, want, str(ov))


def case_narrow_buckets(lib, oracle_lib, example, goldens, monkeypatch, shift=4):
    """The seed-cluster grid with buckets of 2^shift rows instead of 2^12: on the 20 k-row example index a seed's window then
    spans hundreds of buckets (the lane that adds a seed walks them one after the other), clusters move from bucket to bucket as
    they grow, and every bucket holds a cluster or none -- per event against the oracle's set, then a batch."""
    monkeypatch.setenv("UNC_BUCKET_SHIFT", str(shift))
    ix = capi.Index(example["prefix"], lib=lib)
    monkeypatch.delenv("UNC_BUCKET_SHIFT", raising=False)
    case_trace_matches_oracle_every_event(lib, oracle_lib, example, goldens, dev_index=ix)
    oix = oracle_lib.Index(example["prefix"])
    n = 8
    off = goldens["sim_offsets"][:n + 1].copy()
    raw = goldens["sim_signal"][:int(off[n])]
    cal = capi.make_calib(n, CAL_RANGE, CAL_OFFSET, CAL_DIGITISATION)
    hits = capi.Mapper(ix, n_slots=3).map_batch(raw, off, cal)
    assert_hits_equal(hits, oracle_hits(oix, raw, off, cal), "narrow buckets")


def case_loud_overflows(lib, oracle_lib, example, goldens):
    """Device scratch that is too small is REPORTED per read (unc_hit_t.status) and by the call's return code -- never a silent
    wrong answer: a per-event seed list of one entry (UNC_READ_SEED_OVERFLOW); on the chunked path, chunk lengths that could fill the
    rolling normaliser (the reference's #SKIP branch, mapper.cpp:336-351: out of scope) are refused at creation.  Reads that did not
    overflow still answer as the oracle does."""
    dev_index = _index(lib, example)
    oix = oracle_lib.Index(example["prefix"])
    n = 4
    off = goldens["sim_offsets"][:n + 1].copy()
    raw = goldens["sim_signal"][:int(off[n])]
    cal = capi.make_calib(n, CAL_RANGE, CAL_OFFSET, CAL_DIGITISATION)
    m = capi.Mapper(dev_index, n_slots=3, max_seed_paths=1)
    with pytest.raises(RuntimeError):
        m.map_batch(raw, off, cal)                       # the call itself fails ...
    hits = m.map_batch(raw, off, cal, allow_overflow=True)
    want = oracle_hits(oix, raw, off, cal)
    bad = (hits["status"] & 2) != 0
    assert bad.any() and not (hits["status"] & ~np.uint32(2)).any()      # ... and says which reads, and why
    assert not hits["mapped"][bad].any()
    ok = np.flatnonzero(~bad)
    assert_hits_equal(hits[ok], [want[i] for i in ok], "reads without seed overflow")
    # chunked path: the reference's #SKIP branch (a ring of 6000 unread events, mapper.cpp:336-351) is out of scope, formally: chunks
    # long enough to reach it are refused when the pool is created; 3 s chunks (12 000 samples, at most 6000 events) are the limit
    p = capi.default_params(lib)
    p.chunk_time = 15.0
    with pytest.raises(capi.UncalledHipError, match="SKIP"):
        capi.Realtime(dev_index, 1, p)
    p.chunk_time = 3.0
    capi.Realtime(dev_index, 1, p).close()
    p.chunk_time = 3.0 + 1.0 / 4000.0
    with pytest.raises(capi.UncalledHipError):
        capi.Realtime(dev_index, 1, p)


# chunked-path sets: (parameter overrides, chunk length in samples)
CHUNK_VARIANTS = [
    (dict(threshold1=1.7, threshold2=8.0, peak_height=0.35, min_mean=55.0, max_mean=130.0), 4000),
    (dict(min_seed_prob=-3.2, max_consec_stay=3, max_stay_frac=0.25), 2000),         # half-second chunks
    (dict(min_map_len=15, min_mean_conf=3.0, min_top_conf=1.2, max_events=350), 1000),
]


def case_chunked_variants(lib, oracle_lib, example, goldens, n_channels=2, n_reads=6):
    """The chunked path on parameter sets away from the defaults and with other chunk lengths (the detector, the event
    profiler, the rolling normaliser and the mapper all see different event streams): device vs oracle, per read."""
    from uncalled_amd.realtime import MapPoolOrd
    po = oracle_lib
    dev_index = _index(lib, example)
    oix = po.Index(example["prefix"])
    off = goldens["sim_offsets"]
    reads = [(example["signal"], (example["range"], example["offset"], example["digitisation"]))]
    for i in range(n_reads - 1):
        reads.append((goldens["sim_signal"][int(off[i]):int(off[i + 1])], (CAL_RANGE, CAL_OFFSET, CAL_DIGITISATION)))
    names = dev_index.seq_names()
    for ov, chunk_len in CHUNK_VARIANTS:
        p = variant_params(capi.default_params(lib), ov)
        p.chunk_time = chunk_len / p.sample_rate
        pool = MapPoolOrd(dev_index, n_channels=n_channels, params=p)
        assert pool.chunk_len == chunk_len
        oms = [po.Mapper(oix, to_oracle_params(p)) for _ in range(n_channels)]
        want, got, fate = {}, {}, {}
        for i, (raw, cal) in enumerate(reads):
            pool.add_read(i % n_channels, i, raw, cal, key=i)
            want[i], used = oms[i % n_channels].chunk_read(po.calibrate(raw, *cal), chunk_len)
            fate[i] = (used, oms[i % n_channels].rt_ended())
        rounds = 0
        while pool.running():
            for key, r in pool.update():
                got[key] = r
            rounds += 1
            assert rounds < 4000
        for i in range(len(reads)):
            h, o = got[i]["hit"], want[i]
            assert int(h["status"]) == 0
            assert capi.hit_paf_cols(h, names) == po.hit_paf_cols(o, oix.ref_names()), (ov, chunk_len, i)
            for f in ("event_i", "n_nbr", "n_sa", "n_lf", "notes"):
                assert int(h[f]) == int(o[f]), (ov, chunk_len, i, f)
            assert got[i]["state"] == (capi.RT_MAPPED if o["mapped"] else capi.RT_FAILED), (ov, chunk_len, i)
            assert (pool.chunks_used[i], bool(got[i]["ended"])) == fate[i], (ov, chunk_len, i)       # chunks the read was given, Paf::ENDED


def assert_rt_taps_equal(a, ring_a, b, ring_b, what, nan_is_nan=False):
    """stage tap of the chunked path (unc_rt_tap_t layout): detector counters, profiler window + queue, rolling normaliser + ring.
    nan_is_nan: where BOTH sides hold a NaN the two count as equal whatever their bits (the sign of a NaN an operation generates is
    the platform's); everything else stays bit for bit"""
    def same(x, y):
        x, y = np.atleast_1d(x), np.atleast_1d(y)
        eq = x.view("u%d" % x.itemsize) == y.view("u%d" % y.itemsize)
        return bool(np.all(eq | (np.isnan(x) & np.isnan(y)) if nan_is_nan else eq))
    for f in ("det_t", "det_total_events", "norm_n", "norm_wr", "prof_n", "prof_to_mask", "prof_queued"):
        assert a[f] == b[f], (what, f, a[f], b[f])
    assert a["det_len_sum"] == b["det_len_sum"] or (nan_is_nan and same(np.float32(a["det_len_sum"]), np.float32(b["det_len_sum"]))), \
        (what, "det_len_sum", a["det_len_sum"], b["det_len_sum"])
    for f in ("norm_mean", "norm_varsum", "prof_mean", "prof_varsum"):
        assert same(np.float64(a[f]), np.float64(b[f])), (what, f, a[f], b[f])
    q = int(a["prof_queued"])
    assert same(a["prof_queue"][:q], b["prof_queue"][:q]), (what, "prof_queue")
    n = int(a["norm_n"])
    assert same(ring_a[:n], ring_b[:n]), (what, "ring")


def case_chunked_stage_tap(lib, oracle_lib, example, goldens, n_reads=8, chunk_len=4000, cut=None):
    """Below the PAF of the chunked path: after every read of a channel the EventDetector's counters, the EventProfiler's
    25-event window (mean / varsum / mask countdown / queued events) and the rolling 6000-event Normalizer (mean / varsum /
    write position / ring contents) of the device equal the oracle's bit for bit -- a masking or normalisation slip that
    cancelled out in the coordinates would show here.  (tests/test_oracle.py pins the oracle's tap against the reference's.)
    chunk_len: samples per chunk.  With 4000 the channel's state is always stored and loaded at the same phase of the detector's
    16-slot ring of sums and of its 13-sample window; 37 is a multiple of neither, so the hand-over from chunk to chunk meets every
    phase of both (with `cut`, the samples a read is cut to, such a run stays short; max_chunks stays at its default of 10^6, so
    it is never the host that ends a read)."""
    from uncalled_amd.realtime import MapPoolOrd
    po = oracle_lib
    dev_index = _index(lib, example)
    oix = po.Index(example["prefix"])
    p = capi.default_params(lib)
    p.chunk_time = chunk_len / p.sample_rate
    pool = MapPoolOrd(dev_index, n_channels=1, params=p)
    assert pool.chunk_len == chunk_len
    om = po.Mapper(oix, to_oracle_params(p))
    off = goldens["sim_offsets"]
    reads = [(example["signal"], (example["range"], example["offset"], example["digitisation"]))]
    for i in range(n_reads - 1):
        reads.append((goldens["sim_signal"][int(off[i]):int(off[i + 1])], (CAL_RANGE, CAL_OFFSET, CAL_DIGITISATION)))
    reads = [(raw[:cut], cal) for raw, cal in reads]
    for i, (raw, cal) in enumerate(reads):
        pool.add_read(0, i, raw, cal, key=i)
    done = 0
    rounds = 0
    phases = (set(), set())
    while pool.running():
        for key, r in pool.update():
            raw, cal = reads[key]
            om.chunk_read(po.calibrate(raw, *cal), chunk_len)
            (ta, ra), (tb, rb) = pool.rt.tap_channel(0), om.rt_tap()
            assert_rt_taps_equal(ta, ra, tb, rb, "read %d" % key)
            # the read went past the point where the profiler releases events: the tap has a normaliser to compare
            assert int(tb["prof_n"]) == 25 and int(tb["norm_n"]) > 0 and int(tb["det_total_events"]) > 25, (key, tb)
            if cut is not None:
                # the device's detector took every sample of every chunk the read was given (t starts at 1); each chunk but the
                # last handed the state over, at these phases of the 16-slot ring and of the 13-sample window
                used = int(pool.chunks_used[key])
                assert int(ta["det_t"]) == min(used * chunk_len, len(raw)) + 1, (key, ta["det_t"], used)
                for k in range(1, used):
                    phases[0].add(k * chunk_len % 16)
                    phases[1].add(k * chunk_len % 13)
            done += 1
        rounds += 1
        assert rounds < 1000
    assert done == n_reads
    if cut is None:
        assert int(tb["norm_n"]) == 6000       # (the ring has wrapped by then)
    else:
        assert len(phases[0]) == 16 and len(phases[1]) == 13, phases       # a read may be decided early: the run as a whole met every phase


def fuzz_reference(tmp_path):
    """the second reference of tests/dev/fuzz_parity.py: three contigs of 60 kb, loose thresholds (many children per event)"""
    from uncalled_amd.build_index import build_from_codes, synthetic_genome
    names, lens, codes = synthetic_genome(3, 60000, seed=77)
    prefix = tmp_path / "fz"
    if not (tmp_path / "fz.sa").exists():
        build_from_codes(prefix, names, [""] * 3, lens, codes)
        (tmp_path / "fz.uncl").write_text("default\t-10.07,-4.6,-4.0,-3.6,-3.3,-3.1\t0.3\t115.000\n")
    return prefix, codes, lens


def case_unsorted_stream_past_one_block(lib, oracle_lib, tmp_path):
    """max_paths = 1000 with events of many children of sources: the unsorted key stream holds more than 512 keys and is sorted IN
    PLACE in room for exactly max_paths keys.  Round 3's first form of that sort stored whole 512-key blocks, padding included, i.e.
    past the stream's end into the children's info words (found by tests/dev/fuzz_parity.py, seed 2085: a read unmapped that the
    reference maps; the emulator's bounds checks, UNC_SIM_CHECK, now fail on such a store).  The fuzz case, against the oracle."""
    from tools.simulate_reads import simulate_reads
    prefix, codes, lens = fuzz_reference(tmp_path)
    sim = simulate_reads(codes, lens, 4, seed=2085, read_bases=490, off_target=0.0, dwell_mean=11.29495188046118, noise_sd=1.030862943416349)
    p = capi.default_params(lib)
    for k, v in dict(min_rep_len=1, max_rep_copy=28, max_paths=1000, max_consec_stay=2, max_events=2000, max_stay_frac=0.4174584150314331,
                     min_seed_prob=-4.121715545654297, threshold1=1.4309371709823608, threshold2=9.04516315460205,
                     peak_height=0.31874945759773254, min_map_len=27, min_mean_conf=7.31113862991333, min_top_conf=1.9158369302749634).items():
        setattr(p, k, v)
    cal = capi.make_calib(4, CAL_RANGE, CAL_OFFSET, CAL_DIGITISATION)
    ix = capi.Index(prefix, lib=lib)
    hits = capi.Mapper(ix, params=p, n_slots=2, n_waves=2).map_batch(sim["signal"], sim["offsets"], cal)
    want = oracle_hits(oracle_lib.Index(prefix), sim["signal"], sim["offsets"], cal, to_oracle_params(p), fresh_mapper_per_read=True)
    assert_hits_equal(hits, want, "unsorted stream of more than one block")
    assert int(hits["mapped"].sum()) == 2 and (hits["n_nbr"] / np.maximum(hits["event_i"], 1)).min() > 400


CARRY_OVER_PARAMS = dict(max_paths=60, max_rep_copy=2, max_chunks=2)      # with chunks of 8000 samples


def carry_over_data(tmp_path):
    """the reference and reads of tests/dev/fuzz_parity.py's seed 5007 (chunked mode): (index prefix, simulated reads, n)"""
    from tools.simulate_reads import simulate_reads
    prefix, codes, lens = fuzz_reference(tmp_path)
    rng = np.random.default_rng(5007)
    n = int(rng.integers(2, 6))
    sim = simulate_reads(codes, lens, n, seed=5007, read_bases=int(rng.integers(300, 1500)), off_target=float(rng.choice([0.0, 0.3, 1.0])),
                         dwell_mean=float(rng.uniform(6.0, 12.0)), noise_sd=float(rng.uniform(0.5, 3.0)))
    assert n == 4
    return prefix, sim, n


def case_chunked_flags_carry_over(lib, oracle_lib, tmp_path):
    """A channel is one Mapper, and Mapper::new_read does not clear sources_added_ (mapper.cpp:88,612-623: the flags are only
    cleared in a branch a full path buffer never reaches).  With a small max_paths a read therefore sees the flags its
    predecessor on the channel left behind; the chunked path reproduces that (found by tests/dev/fuzz_parity.py, seed 5007: the
    fourth read of a channel did two get_neighbor calls more when the flags were cleared).  Reads of the fuzz case, one channel;
    the scenario is checked to be one where the carry-over matters (a fresh Mapper per read answers differently)."""
    from uncalled_amd.realtime import MapPoolOrd
    po = oracle_lib
    prefix, sim, n = carry_over_data(tmp_path)
    ix = capi.Index(prefix, lib=lib)
    oix = po.Index(prefix)
    p = capi.default_params(lib)
    p.max_paths, p.max_rep_copy, p.max_chunks, p.chunk_time = 60, 2, 2, 8000 / p.sample_rate
    pool = MapPoolOrd(ix, n_channels=1, params=p)
    om = po.Mapper(oix, to_oracle_params(p))
    om.set_max_chunks(2)
    off = sim["offsets"]
    cal = (CAL_RANGE, CAL_OFFSET, CAL_DIGITISATION)
    want, alone = [], []
    for i in range(n):
        raw = sim["signal"][int(off[i]):int(off[i + 1])]
        pool.add_read(0, i, raw, cal, key=i)
        want.append(om.chunk_read(po.calibrate(raw, *cal), 8000)[0])
        fresh = po.Mapper(oix, to_oracle_params(p))
        fresh.set_max_chunks(2)
        alone.append(fresh.chunk_read(po.calibrate(raw, *cal), 8000)[0])
    got = {}
    while pool.running():
        for key, r in pool.update():
            got[key] = r["hit"]
    names_dev = ix.seq_names()
    for i in range(n):
        assert capi.hit_paf_cols(got[i], names_dev) == po.hit_paf_cols(want[i], oix.ref_names()), i
        for f in ("event_i", "n_nbr", "n_sa", "n_lf", "notes"):
            assert int(got[i][f]) == int(want[i][f]), (i, f)
    assert any(int(want[i]["n_nbr"]) != int(alone[i]["n_nbr"]) or int(want[i]["event_i"]) != int(alone[i]["event_i"]) for i in range(1, n))


def case_chunked_realtime_path(lib, oracle_lib, example, goldens, n_channels=3, n_reads=9, max_chunks=None, long_read=False):
    """Config 5's path: reads replayed chunk by chunk over a few channels (MapPoolOrd semantics) through
    unc_rt_process_chunks; per-channel state persists across chunks AND reads.  Checked against the oracle fed the
    same reads in the same per-channel order, and (default max_chunks, channel 0 order) against the reference goldens."""
    from uncalled_amd.realtime import MapPoolOrd
    po = oracle_lib
    dev_index = _index(lib, example)
    oix = po.Index(example["prefix"])
    p = capi.default_params(lib)
    if max_chunks:
        p.max_chunks = max_chunks
    pool = MapPoolOrd(dev_index, n_channels=n_channels, params=p)
    off = goldens["sim_offsets"]
    reads = [(example["signal"], (example["range"], example["offset"], example["digitisation"]))]
    for i in range(n_reads - 1):
        reads.append((goldens["sim_signal"][int(off[i]):int(off[i + 1])], (CAL_RANGE, CAL_OFFSET, CAL_DIGITISATION)))
    if long_read:
        # an off-target read with more events than the 6000-slot normaliser ring holds: the ring wraps inside one read
        from tools.simulate_reads import simulate_reads
        sim = simulate_reads(np.zeros(20000, np.uint8), [20000], 1, seed=9, read_bases=5200, off_target=1.0)
        reads.insert(1, (sim["signal"], (CAL_RANGE, CAL_OFFSET, CAL_DIGITISATION)))
    oms = [po.Mapper(oix) for _ in range(n_channels)]
    for om in oms:
        if max_chunks:
            om.set_max_chunks(max_chunks)
    want, fate = {}, {}
    for i, (raw, cal) in enumerate(reads):
        ch = i % n_channels
        pool.add_read(ch, i, raw, cal, key=i)
        want[i], used = oms[ch].chunk_read(po.calibrate(raw, *cal), 4000)
        fate[i] = (used, oms[ch].rt_ended())
    got = {}
    rounds = 0
    while pool.running():
        for key, r in pool.update():
            got[key] = r
        rounds += 1
        assert rounds < 1000
    names = dev_index.seq_names()
    for i in range(len(reads)):
        h, o = got[i]["hit"], want[i]
        assert int(h["status"]) == 0
        assert capi.hit_paf_cols(h, names) == po.hit_paf_cols(o, oix.ref_names()), i
        for f in ("event_i", "n_nbr", "n_sa", "n_lf", "notes"):
            assert int(h[f]) == int(o[f]), (i, f)
        assert got[i]["state"] == (capi.RT_MAPPED if o["mapped"] else capi.RT_FAILED), i
        assert (pool.chunks_used[i], bool(got[i]["ended"])) == fate[i], i        # chunks the read was given, Paf::ENDED
    if long_read:
        assert int(want[1]["event_i"]) > 6500 and not want[1]["mapped"]
    if n_channels == 1 and not max_chunks and not long_read:
        f = {str(n): j for j, n in enumerate(goldens["hit_fields"])}
        for i in range(len(reads)):
            for name in ("mapped", "rd_st", "rd_en", "rd_len", "rf_st", "rf_en", "matches", "event_i", "n_nbr", "n_lf"):
                assert int(got[i]["hit"][name]) == int(goldens["chunk_hits"][i][f[name]]), (i, name)


def _off_target_chunks(n_samples=11000, chunk_len=4000):
    """one simulated off-target read (it never maps), cut to n_samples: (signal, calibration, [(offset, length)] of its chunks)"""
    from tools.simulate_reads import simulate_reads
    sig = simulate_reads(np.zeros(20000, np.uint8), [20000], 1, seed=9, read_bases=5200, off_target=1.0)["signal"][:n_samples]
    assert sig.size == n_samples
    return sig, (CAL_RANGE, CAL_OFFSET, CAL_DIGITISATION), [(o, min(chunk_len, n_samples - o)) for o in range(0, n_samples, chunk_len)]


def _rt_chunk(channel, read_number, flags, offset, n_samples, cal):
    ch = np.zeros(1, dtype=capi.RT_CHUNK)
    ch["channel"], ch["read_number"], ch["flags"], ch["offset"], ch["n_samples"] = channel, read_number, flags, offset, n_samples
    ch["calib"] = capi.make_calib(1, *cal)[0]
    return ch


def _rt_flags(k, n):
    return (capi.RT_FIRST if k == 0 else 0) | (capi.RT_LAST if k == n - 1 else 0)


def case_chunked_rejected_call_leaves_no_trace(lib, oracle_lib, example, goldens, n_channels=2):
    """A call that unc_rt_process_chunks rejects (UNC_ERR_ARG) changes nothing: object B gets, before the 2nd and before the 3rd
    chunk of a read on channel 0, calls that must fail -- the read's valid next chunk first, the offending entry after it -- and
    goes on to answer every valid call byte for byte as its undisturbed twin A, up to max_chunks = 3 on the third chunk; the final
    record is the oracle's.  (A library that admits chunk 0 before it rejects the call counts the chunk twice: rd_len grows and
    the read fails one chunk early.)  With two channels the three entries of the duplicate-channel call are already refused by
    their number; with three channels the duplicate itself is."""
    po = oracle_lib
    dev_index = _index(lib, example)
    p = capi.default_params(lib)
    p.max_chunks = 3
    chunk_len = int(p.chunk_time * p.sample_rate)
    assert chunk_len == 4000
    sig, cal, spans = _off_target_chunks(11000, chunk_len)
    A, B = (capi.Realtime(dev_index, n_channels=n_channels, params=p) for _ in range(2))
    valid = [_rt_chunk(0, 7, _rt_flags(k, len(spans)), o, n, cal) for k, (o, n) in enumerate(spans)]
    other = _rt_chunk(1, 8, capi.RT_FIRST, 0, 1000, cal)
    twice = ([other, other], "more chunks than channels" if n_channels == 2 else "two chunks for channel 1 in one call")
    beyond = ([_rt_chunk(n_channels, 8, capi.RT_FIRST, 0, 1000, cal)], "chunk 1: channel %d out of range" % n_channels)
    too_long = ([_rt_chunk(1, 8, capi.RT_FIRST, 0, chunk_len + 1, cal)], "chunk 1 longer than chunk_time \\* sample_rate")
    bad_calls = {1: [twice, beyond], 2: [too_long, twice]}
    last = None
    for k, ch in enumerate(valid):
        for extra, message in bad_calls.get(k, []):
            with pytest.raises(capi.UncalledHipError, match=message):
                B.process_chunks(np.concatenate([ch] + extra), raw_i16=sig)
        a, b = A.process_chunks(ch, raw_i16=sig), B.process_chunks(ch, raw_i16=sig)
        assert a.tobytes() == b.tobytes(), (k, a, b)
        if k == 1:
            assert a[0]["state"] == capi.RT_MAPPING      # the read is still open when the second round of bad calls comes
        last = b[0]
    assert last["state"] == capi.RT_FAILED and not last["ended"]      # max_chunks on the third chunk, not the last-chunk exit
    oix = po.Index(example["prefix"])
    om = po.Mapper(oix)
    om.set_max_chunks(3)
    want, used = om.chunk_read(po.calibrate(sig, *cal), chunk_len)
    assert (used, om.rt_ended()) == (3, False)
    assert capi.hit_paf_cols(last["hit"], dev_index.seq_names()) == po.hit_paf_cols(want, oix.ref_names())
    for f in ("event_i", "n_nbr", "n_sa", "n_lf", "notes"):
        assert int(last["hit"][f]) == int(want[f]), f
    assert int(last["hit"]["status"]) == 0 and not want["mapped"]
    # channel 1 never started a read: nothing of the rejected calls' entries was admitted
    assert B.process_chunks(_rt_chunk(1, 8, 0, 0, 1000, cal), raw_i16=sig)[0]["state"] == capi.RT_IGNORED
    A.close()
    B.close()


def case_chunked_ignored_chunks(lib, oracle_lib, example, goldens):
    """UNC_RT_IGNORED: a chunk without UNC_RT_FIRST on an idle channel, and a chunk of read 6 on a channel that is mapping read 5,
    give an empty result (hit.rid = -1) and leave read 5 to finish as on an undisturbed twin -- also when the ignored chunk comes
    first in a call, so that the launch's first block is not the call's first chunk."""
    dev_index = _index(lib, example)
    sig, cal, spans = _off_target_chunks(11000, 4000)
    R, T = (capi.Realtime(dev_index, n_channels=2) for _ in range(2))
    ignored = np.zeros(1, dtype=capi.RT_RESULT)
    ignored["state"], ignored["hit"]["rid"] = capi.RT_IGNORED, -1
    valid = [_rt_chunk(0, 5, _rt_flags(k, len(spans)), o, n, cal) for k, (o, n) in enumerate(spans)]
    idle = _rt_chunk(1, 3, 0, 0, 2000, cal)
    assert R.process_chunks(idle, raw_i16=sig).tobytes() == ignored.tobytes()
    first = R.process_chunks(valid[0], raw_i16=sig)
    assert first.tobytes() == T.process_chunks(valid[0], raw_i16=sig).tobytes() and first[0]["state"] == capi.RT_MAPPING
    assert R.process_chunks(_rt_chunk(0, 6, 0, 4000, 4000, cal), raw_i16=sig).tobytes() == ignored.tobytes()
    both = R.process_chunks(np.concatenate([idle, valid[1]]), raw_i16=sig)
    assert both[:1].tobytes() == ignored.tobytes()
    assert both[1:].tobytes() == T.process_chunks(valid[1], raw_i16=sig).tobytes() and both[1]["state"] == capi.RT_MAPPING
    both = R.process_chunks(np.concatenate([valid[2], _rt_chunk(1, 6, capi.RT_LAST, 0, 2000, cal)]), raw_i16=sig)
    assert both[1:].tobytes() == ignored.tobytes()
    assert both[:1].tobytes() == T.process_chunks(valid[2], raw_i16=sig).tobytes()
    assert both[0]["state"] == capi.RT_FAILED and both[0]["ended"] and int(both[0]["hit"]["rd_len"]) > 0      # given up at its last chunk
    R.close()
    T.close()


def case_cluster_overflow_remap(lib, oracle_lib, example, goldens):
    """The reference's SeedTracker is unbounded; reads that outgrow the per-slot cluster array are re-mapped on the device
    with more room until they fit.  Forced here with an absurdly small array."""
    dev_index = _index(lib, example)
    oix = oracle_lib.Index(example["prefix"])
    n = 6
    off = goldens["sim_offsets"][:n + 1].copy()
    raw = goldens["sim_signal"][:int(off[n])]
    cal = capi.make_calib(n, CAL_RANGE, CAL_OFFSET, CAL_DIGITISATION)
    hits = capi.Mapper(dev_index, n_slots=2, max_clusters=8).map_batch(raw, off, cal)
    assert_hits_equal(hits, oracle_hits(oix, raw, off, cal), "remap")


def case_wide_sort_keys(lib, oracle_lib, example, goldens, monkeypatch, n=10):
    """References too large for the packed 64-bit sort key (GRCh38-sized: seq_len x k-mer range x 2^16 > 2^64) take
    the 128-bit key path; forced here through UNC_WIDE_KEYS on the small index."""
    monkeypatch.setenv("UNC_WIDE_KEYS", "1")
    ix = capi.Index(example["prefix"], lib=lib)
    monkeypatch.delenv("UNC_WIDE_KEYS", raising=False)
    oix = oracle_lib.Index(example["prefix"])
    off = goldens["sim_offsets"][:n + 1].copy()
    raw = goldens["sim_signal"][:int(off[n])]
    cal = capi.make_calib(n, CAL_RANGE, CAL_OFFSET, CAL_DIGITISATION)
    hits = capi.Mapper(ix, n_slots=3).map_batch(raw, off, cal)
    assert_hits_equal(hits, oracle_hits(oix, raw, off, cal), "wide keys")


def case_sliced_scheduler(lib, oracle_lib, example, goldens, max_paths=10000, slice_events=37, n_slots=5, n_waves=2, n_reads=24):
    """More reads in flight than wavefronts (DevSched): reads are parked after `slice_events` events and resumed later,
    possibly by another wavefront; answers and work counters must not change (also with the max_paths cut-off, whose
    stale sources_added_ flags travel with the parked read)."""
    dev_index = _index(lib, example)
    p = capi.default_params(dev_index.L)
    p.max_paths = max_paths
    off_all = goldens["sim_offsets"]
    raw = goldens["sim_signal"][:int(off_all[n_reads])]
    off = off_all[:n_reads + 1].copy()
    cal = capi.make_calib(n_reads, CAL_RANGE, CAL_OFFSET, CAL_DIGITISATION)
    m = capi.Mapper(dev_index, params=p, n_slots=n_slots, n_waves=n_waves, slice_events=slice_events)
    hits = m.map_batch(raw, off, cal)
    again = m.map_batch(raw, off, cal)          # the rings are re-initialised per batch
    for name in capi.RESULT_FIELDS:
        assert np.array_equal(again[name], hits[name]), name
    oix = oracle_lib.Index(example["prefix"])
    assert_hits_equal(hits, oracle_hits(oix, raw, off, cal, to_oracle_params(p), fresh_mapper_per_read=True), "sliced")


def case_scheduler_rings_per_xcd(lib, oracle_lib, example, goldens, n_reads=24, slice_events=37):
    """One pair of scheduler rings per XCD (SchedCtl): a slot stays with the wavefronts of one XCD, which park and resume its reads without
    an L2 write-back / invalidate.  512 slots divide into eight shares of 64: the library settles on the device's XCD count (8 on the
    MI355X; the emulator deals its workgroups to eight XCDs from XCD 3 on, so the shares in use are not the first), a mapper told
    sched_parts=1 keeps one pair for the device, and both answer as the oracle does; a share of fewer than 64 slots falls back to one pair."""
    dev_index = _index(lib, example)
    off_all = goldens["sim_offsets"]
    raw = goldens["sim_signal"][:int(off_all[n_reads])]
    off = off_all[:n_reads + 1].copy()
    cal = capi.make_calib(n_reads, CAL_RANGE, CAL_OFFSET, CAL_DIGITISATION)
    oix = oracle_lib.Index(example["prefix"])
    want = oracle_hits(oix, raw, off, cal, fresh_mapper_per_read=True)
    m = capi.Mapper(dev_index, n_slots=512, n_waves=8, slice_events=slice_events, pool_chunks=256)
    parts = m.sched_parts()
    assert parts in (1, 8), parts               # (1: a device, or a partition mode, that shows one XCD)
    hits = m.map_batch(raw, off, cal)
    again = m.map_batch(raw, off, cal)
    assert_hits_equal(hits, want, "rings per XCD")
    m1 = capi.Mapper(dev_index, n_slots=512, n_waves=8, slice_events=slice_events, pool_chunks=256, sched_parts=1)
    assert m1.sched_parts() == 1
    hits1 = m1.map_batch(raw, off, cal)
    for name in capi.RESULT_FIELDS:
        assert np.array_equal(again[name], hits[name]) and np.array_equal(hits1[name], hits[name]), name
    m2 = capi.Mapper(dev_index, n_slots=256, n_waves=8, slice_events=slice_events, pool_chunks=256)      # shares of 32 slots
    assert m2.sched_parts() == 1
    with pytest.raises(capi.UncalledHipError):
        capi.Mapper(dev_index, n_slots=512, n_waves=8, slice_events=slice_events, pool_chunks=256, sched_parts=3)
    return parts


def case_cluster_pool_pressure(lib, oracle_lib, example, goldens, pool_chunks=2, n_waves=2, n_reads=12):
    """The nodes of all seed-cluster sets come from one pool.  With fewer chunks than reads in flight some reads find it
    dry; with a tiny allowance of nodes some outgrow that: both are mapped again after the batch (with fewer reads sharing
    the pool; with a larger allowance) and every read still answers as the oracle does.  A roomy pool needs no second pass."""
    dev_index = _index(lib, example)
    off_all = goldens["sim_offsets"]
    raw = goldens["sim_signal"][:int(off_all[n_reads])]
    off = off_all[:n_reads + 1].copy()
    cal = capi.make_calib(n_reads, CAL_RANGE, CAL_OFFSET, CAL_DIGITISATION)
    oix = oracle_lib.Index(example["prefix"])
    want = oracle_hits(oix, raw, off, cal, fresh_mapper_per_read=True)
    m = capi.Mapper(dev_index, n_slots=3 * n_waves, n_waves=n_waves, slice_events=60, pool_chunks=pool_chunks)
    assert m.geometry() == dict(n_waves=n_waves, n_slots=3 * n_waves, slice_events=60, pool_chunks=pool_chunks, max_clusters=1 << 20)
    hits = m.map_batch(raw, off, cal)
    assert m.last_remap()[0] > 0            # 3 * n_waves reads in flight, pool_chunks < that many chunks
    assert_hits_equal(hits, want, "pool pressure")
    m2 = capi.Mapper(dev_index, n_slots=3 * n_waves, n_waves=n_waves, slice_events=60, pool_chunks=64, max_clusters=16)
    hits2 = m2.map_batch(raw, off, cal)      # one leaf per read: the ones with more than 64 clusters outgrow the directory
    assert m2.last_remap()[0] > 0
    m3 = capi.Mapper(dev_index, n_slots=3 * n_waves, n_waves=n_waves, slice_events=60, pool_chunks=64)
    hits3 = m3.map_batch(raw, off, cal)
    assert m3.last_remap()[0] == 0
    # both causes in one batch: reads that find the pool dry run again with fewer fellows, reads past their own allowance
    # (max_clusters / 4 nodes) with a larger one -- and a read may meet one cause after the other
    m4 = capi.Mapper(dev_index, n_slots=3 * n_waves, n_waves=n_waves, slice_events=60, pool_chunks=pool_chunks, max_clusters=16)
    hits4 = m4.map_batch(raw, off, cal)
    assert m4.last_remap()[0] > 0
    for name in capi.RESULT_FIELDS:
        assert np.array_equal(hits[name], hits2[name]) and np.array_equal(hits[name], hits3[name]) and np.array_equal(hits[name], hits4[name]), name
    # the pool is sized by NEED (unc_mapper_pool_usage): a named size stays as it is and its high-water mark is reported ...
    u = m.pool_usage()
    assert u["chunks"] == pool_chunks and u["resizes"] == 0 and u["high_water_ever"] == pool_chunks          # it ran dry: every chunk was out
    u3 = m3.pool_usage()
    assert u3["chunks"] == 64 and 0 < u3["high_water_last_batch"] <= 3 * n_waves and u3["resizes"] == 0      # at most a chunk per read in flight here
    # ... the default starts from the rule of thumb and is then cut to four times the most chunks that were out at once when it holds more
    # than eight times that (never below one per slot / 16; four times, since round 5 saw one batch's peak move by tens of per cent
    # between launches) -- but only by a batch that FILLED the slots (round-5 advice: a warm-up call or a handful of reads must not cut a
    # pool sized for a full load of reads in flight).  32 slots, twelve reads: the rule of thumb gives 256 chunks and the batch leaves them
    m5 = capi.Mapper(dev_index, n_slots=32, n_waves=n_waves, slice_events=60)
    before = m5.geometry()["pool_chunks"]
    hits5 = m5.map_batch(raw, off, cal)
    u5 = m5.pool_usage()
    assert before == 256 and 0 < u5["high_water_ever"] <= n_reads and m5.last_remap()[0] == 0
    assert (u5["chunks"], u5["resizes"]) == ((256, 0) if n_reads < 32 else (max(32, 4 * u5["high_water_ever"]), 1)), u5
    # as many slots as reads (at most six): the batch fills the slots, and the pool (eight chunks per slot by the rule of thumb) is cut
    # by the rule above whenever the rule says so
    ns7 = min(6, n_reads)
    m7 = capi.Mapper(dev_index, n_slots=ns7, n_waves=min(n_waves, ns7), slice_events=60)
    before7 = m7.geometry()["pool_chunks"]
    hits7 = m7.map_batch(raw, off, cal)
    u7 = m7.pool_usage()
    need = max(16, 4 * u7["high_water_ever"])        # never below 16 chunks / one chunk per slot
    want7 = need if 2 * need < before7 else before7
    assert before7 == max(16, 8 * ns7) and 0 < u7["high_water_ever"] <= ns7, (before7, u7)
    assert u7["chunks"] == want7 and u7["resizes"] == (1 if want7 != before7 else 0), (before7, u7, want7)
    assert m7.last_remap()[0] == 0
    hits8 = m7.map_batch(raw, off, cal)              # the second batch finds the pool sized and leaves it
    assert m7.pool_usage()["resizes"] == u7["resizes"] and m7.pool_usage()["chunks"] == u7["chunks"] and m7.last_remap()[0] == 0
    for name in capi.RESULT_FIELDS:
        assert np.array_equal(hits[name], hits7[name]) and np.array_equal(hits[name], hits8[name]), name
    hits6 = m5.map_batch(raw, off, cal)
    assert m5.pool_usage()["resizes"] == u5["resizes"] and m5.pool_usage()["chunks"] == u5["chunks"] and m5.last_remap()[0] == 0
    for name in capi.RESULT_FIELDS:
        assert np.array_equal(hits[name], hits5[name]) and np.array_equal(hits[name], hits6[name]), name


def case_big_forests(lib, oracle_lib, example, goldens, tmp_path, monkeypatch, wide_too=True):
    """Path forests of more than 512 children per event on the small index (permissive thresholds): the sorts beyond one
    register block -- 512-key blocks + stages through memory -- in both key modes, against the oracle."""
    import shutil
    for suf in (".amb", ".ann", ".bwt", ".pac", ".sa"):
        shutil.copy(str(example["prefix"]) + suf, str(tmp_path / ("loose" + suf)))
    (tmp_path / "loose.uncl").write_text("default\t-10.07,-5.5,-5.0,-4.6,-4.3,-4.1\t0.3\t115.000\n")
    prefix = tmp_path / "loose"
    n = 3
    off_all = goldens["sim_offsets"]
    raw = np.concatenate([goldens["sim_signal"][int(off_all[i]):int(off_all[i]) + 5000] for i in range(n)])
    off = (np.arange(n + 1) * 5000).astype(np.uint64)
    cal = capi.make_calib(n, CAL_RANGE, CAL_OFFSET, CAL_DIGITISATION)
    want = oracle_hits(oracle_lib.Index(prefix), raw, off, cal)
    for wide in ((False, True) if wide_too else (False,)):
        if wide:
            monkeypatch.setenv("UNC_WIDE_KEYS", "1")
        ix = capi.Index(prefix, lib=lib)
        hits = capi.Mapper(ix, n_slots=n).map_batch(raw, off, cal)
        assert_hits_equal(hits, want, "big forests, wide keys" if wide else "big forests")
        assert (hits["n_nbr"] / np.maximum(hits["event_i"], 1)).min() > 1000        # ~600 parents, well over 512 children per event
    monkeypatch.delenv("UNC_WIDE_KEYS", raising=False)


def case_mid_reference(lib, oracle_lib, tmp_path, n=3, genome=800000, cut=8000):
    """A reference large enough that few children sit on a k-mer's boundary row (on the 10 kb example index nearly every
    event has one and takes the sort through memory): events with many children then go through the merge that walks its
    output tile in LDS.  Built here (synthetic genome, permissive thresholds), against the oracle."""
    from uncalled_amd.build_index import build_from_codes, synthetic_genome
    from tools.simulate_reads import simulate_reads
    names, lens, codes = synthetic_genome(1, genome, seed=11)
    prefix = tmp_path / "mid"
    build_from_codes(prefix, names, [""], lens, codes)
    (tmp_path / "mid.uncl").write_text("default\t-10.07,-5.5,-5.0,-4.6,-4.3,-4.1\t0.3\t115.000\n")     # permissive: hundreds of children per event
    sim = simulate_reads(codes, lens, n, seed=5)
    off = sim["offsets"]
    raw = np.concatenate([sim["signal"][int(off[i]):int(off[i]) + cut] for i in range(n)])
    o = (np.arange(n + 1) * cut).astype(np.uint64)
    cal = capi.make_calib(n, CAL_RANGE, CAL_OFFSET, CAL_DIGITISATION)
    hits = capi.Mapper(capi.Index(prefix, lib=lib), n_slots=n).map_batch(raw, o, cal)
    want = oracle_hits(oracle_lib.Index(prefix), raw, o, cal)
    assert_hits_equal(hits, want, "mid reference")
    assert (hits["n_nbr"] / np.maximum(hits["event_i"], 1)).max() > 300      # events well past the merge threshold


def case_chunked_mid_reference(lib, oracle_lib, tmp_path, n=2, genome=800000, cut=8000, chunk_len=4000, n_channels=2):
    """The chunked path where events have HUNDREDS of children (case_mid_reference's reference and thresholds): the team kernel's own
    sort -- runs repaired by four waves at once, merge tiles dealt to the waves, the leader walking the sorted tiles in the other
    waves' LDS -- only runs for events past the merge threshold, which the 10 kb example index hardly produces.  Chunk by chunk
    against the oracle's chunk path, per-channel state carried from read to read."""
    from uncalled_amd.build_index import build_from_codes, synthetic_genome
    from uncalled_amd.realtime import MapPoolOrd
    from tools.simulate_reads import simulate_reads
    po = oracle_lib
    names, lens, codes = synthetic_genome(1, genome, seed=11)
    prefix = tmp_path / "mid"
    build_from_codes(prefix, names, [""], lens, codes)
    (tmp_path / "mid.uncl").write_text("default\t-10.07,-5.5,-5.0,-4.6,-4.3,-4.1\t0.3\t115.000\n")     # permissive: hundreds of children per event
    sim = simulate_reads(codes, lens, n, seed=5)
    off = sim["offsets"]
    dev_index = capi.Index(prefix, lib=lib)
    oix = po.Index(prefix)
    p = capi.default_params(lib)
    p.chunk_time = chunk_len / p.sample_rate
    pool = MapPoolOrd(dev_index, n_channels=n_channels, params=p)
    oms = [po.Mapper(oix, to_oracle_params(p)) for _ in range(n_channels)]
    cal = (CAL_RANGE, CAL_OFFSET, CAL_DIGITISATION)
    want, fate = {}, {}
    for i in range(n):
        raw = sim["signal"][int(off[i]):int(off[i]) + cut]
        pool.add_read(i % n_channels, i, raw, cal, key=i)
        want[i], used = oms[i % n_channels].chunk_read(po.calibrate(raw, *cal), chunk_len)
        fate[i] = (used, oms[i % n_channels].rt_ended())
    got, rounds = {}, 0
    while pool.running():
        for key, r in pool.update():
            got[key] = r
        rounds += 1
        assert rounds < 1000
    names_dev = dev_index.seq_names()
    for i in range(n):
        h, o = got[i]["hit"], want[i]
        assert int(h["status"]) == 0
        assert capi.hit_paf_cols(h, names_dev) == po.hit_paf_cols(o, oix.ref_names()), i
        for f in ("event_i", "n_nbr", "n_sa", "n_lf", "notes"):
            assert int(h[f]) == int(o[f]), (i, f)
        assert (pool.chunks_used[i], bool(got[i]["ended"])) == fate[i], i
    assert max(int(want[i]["n_nbr"]) / max(int(want[i]["event_i"]), 1) for i in range(n)) > 300      # events well past the merge threshold


def case_same_row_two_kmers(lib, oracle_lib, tmp_path, n=3, seed=5):
    """Two children with the SAME one-row range and DIFFERENT k-mers: BwaIndex::get_base_range starts one row low
    (bwa_index.hpp:172-174), so neighbouring k-mer ranges share a boundary row; the reference walks such a pair in seed_prob order
    (mapper.cpp:543-563), which a narrow sort key cannot express.  The narrow-key walk notices the pair, puts sources_added_ back and
    the event is walked again on 128-bit keys (k_map.hip: WalkState::mixed, phase_S_wide_redo).  On a 3 x 60 kb reference with
    permissive thresholds about one event in a hundred is such an event (none on the bench references' scale cases, none on the 10 kb
    example): the emulator build counts them and the case insists that some were seen."""
    import ctypes
    from uncalled_amd.build_index import build_from_codes, synthetic_genome
    from tools.simulate_reads import simulate_reads
    names, lens, codes = synthetic_genome(3, 60000, seed=77)
    prefix = tmp_path / "fz"
    build_from_codes(prefix, names, [""] * 3, lens, codes)
    (tmp_path / "fz.uncl").write_text("default\t-10.07,-4.6,-4.0,-3.6,-3.3,-3.1\t0.3\t115.000\n")
    try:
        cnt = ctypes.c_ulonglong.in_dll(lib, "unc_sim_wide_redo_count")       # (the emulator build only)
    except ValueError:
        cnt = None
    before = cnt.value if cnt is not None else 0
    dix, oix = capi.Index(prefix, lib=lib), oracle_lib.Index(prefix)
    cal = capi.make_calib(n, CAL_RANGE, CAL_OFFSET, CAL_DIGITISATION)
    for off_target in (0.0, 1.0):
        sim = simulate_reads(codes, lens, n, seed=seed, read_bases=600, off_target=off_target)
        hits = capi.Mapper(dix, n_slots=n).map_batch(sim["signal"], sim["offsets"], cal)
        assert_hits_equal(hits, oracle_hits(oix, sim["signal"], sim["offsets"], cal), "same row, two k-mers (off target %.0f)" % off_target)
    import os
    if cnt is not None and not os.environ.get("UNC_WIDE_KEYS"):        # (with 128-bit keys forced every event is walked on them at once)
        assert cnt.value - before >= 10, "hardly any event took the wide-key redo (%d): the path is untested" % (cnt.value - before)


def case_batch_in_two_halves(lib, oracle_lib, example, goldens, n_reads=6):
    """unc_map_batch_begin / unc_map_batch_end: a batch launched and collected in two calls, two mappers over one index with a batch in
    flight on each (the second begun before the first is collected, as bench.py and a two-mapper worker loop do), host and device
    buffers alike -> the hits of unc_map_batch, which are the oracle's.  A second _begin before the _end, and an _end without a
    _begin, are refused."""
    dev_index = _index(lib, example)
    off_all = goldens["sim_offsets"]
    raw = goldens["sim_signal"][:int(off_all[n_reads])]
    off = off_all[:n_reads + 1].copy()
    cal = capi.make_calib(n_reads, CAL_RANGE, CAL_OFFSET, CAL_DIGITISATION)
    want = oracle_hits(oracle_lib.Index(example["prefix"]), raw, off, cal, fresh_mapper_per_read=True)
    a = capi.Mapper(dev_index, n_slots=4, n_waves=2, slice_events=50)
    b = capi.Mapper(dev_index, n_slots=3, n_waves=3)
    whole = a.map_batch(raw, off, cal)
    assert_hits_equal(whole, want, "unc_map_batch")
    half = n_reads // 2
    off2 = (off[half:] - off[half]).astype(np.uint64)
    raw2 = raw[int(off[half]):]
    for _round in range(2):                    # (twice: a mapper is as good as new after _end)
        a.begin_batch(raw, off, cal)
        b.begin_batch(raw2, off2, cal[half:])  # begun while a's batch is in flight
        with pytest.raises(capi.UncalledHipError):
            a.begin_batch(raw, off, cal)       # one batch per mapper at a time
        ha = a.end_batch()
        hb = b.end_batch()
        for name in capi.RESULT_FIELDS:
            assert np.array_equal(ha[name], whole[name]), name
            assert np.array_equal(hb[name], whole[name][half:]), name
    with pytest.raises(capi.UncalledHipError):
        a.end_batch()                          # nothing begun
    assert_hits_equal(a.map_batch(raw, off, cal), want, "unc_map_batch after the halves")


# ---- calibrations other than the simulators' (tests/helpers.py REGIMES): per value, per read, per channel

def _wide_bounds(lib):
    """default parameters with no event dropped for its mean"""
    p = capi.default_params(lib)
    p.min_mean, p.max_mean = -3.0e38, 3.0e38
    return p


def _assert_events_equal(po, means, moff, info, reads, cals, params, what):
    """every kept mean, both counters, the mean event length and the normaliser's scale / shift of every read against the oracle"""
    for i, (r, c) in enumerate(zip(reads, cals)):
        ev, mel, tot = po.detect_events(po.calibrate(r, *c), params)
        assert info["n_events"][i] == len(ev) and info["total_events"][i] == tot, (what, i, int(info["n_events"][i]), len(ev))
        got = means[int(moff[i]):int(moff[i + 1])]
        assert np.array_equal(got.view(np.uint32), ev["mean"].astype(np.float32).view(np.uint32)), (what, i)
        if tot:
            assert np.float32(info["len_sum"][i] / info["total_events"][i]) == np.float32(mel), (what, i)
        if len(ev):
            _, sc, sh = po.normalize(ev["mean"])
            assert np.float32(sc).tobytes() == np.float32(info["scale"][i]).tobytes(), (what, i)
            assert np.float32(sh).tobytes() == np.float32(info["shift"][i]).tobytes(), (what, i)


def case_calibration_through_event_means(lib, oracle_lib, example):
    """Step signals -- runs of 20 equal samples over the whole int16 range, negative values (u16 above 32767) included -- one read per
    calibration regime in ONE batch: an event inside a run has the run's calibrated value as its mean, so k_events' calibration of each
    read shows value by value (against the numpy restatement), and every event against the oracle.  No event is dropped for its mean."""
    from tests.helpers import REGIMES, calibrate_np, calib_of
    po = oracle_lib
    p = _wide_bounds(lib)
    rng = np.random.default_rng(11)
    reads, cals = [], list(REGIMES.values())
    for _ in cals:
        vals = np.concatenate((rng.integers(-32768, 32768, 100), rng.integers(0, 1024, 20), [0, -1, 1, 32767, -32768, 243, 242, 244, 7, 6]))
        rng.shuffle(vals)
        r = np.repeat(vals, 20).astype(np.int16)
        r[rng.integers(0, r.size, 40)] += 1          # a few runs broken: events that straddle a change
        reads.append(r)
    raw = np.concatenate(reads)
    off = np.concatenate(([0], np.cumsum([r.size for r in reads]))).astype(np.uint64)
    m = capi.Mapper(_index(lib, example), params=p, n_slots=1)
    means, moff, info = m.detect_events(raw, off, calib_of(cals))
    _assert_events_equal(po, means, moff, info, reads, cals, to_oracle_params(p), "step signals")
    for i, (r, c) in enumerate(zip(reads, cals)):
        ev = po.detect_events(po.calibrate(r, *c), to_oracle_params(p))[0]
        st, ln = ev["start"].astype(np.int64), ev["length"].astype(np.int64)
        inside = np.array([ln[j] > 0 and np.all(r[st[j]:st[j] + ln[j]] == r[st[j]]) for j in range(len(ev))], dtype=bool)
        assert inside.sum() >= 100, (i, int(inside.sum()))
        got = means[int(moff[i]):int(moff[i + 1])][inside]
        assert np.array_equal(got.view(np.uint32), calibrate_np(r[st[inside]], *c).view(np.uint32)), i


def case_event_mean_bounds(lib, oracle_lib, example):
    """Identity calibration (pA = the stored sample): steps at exactly min_mean - 1, min_mean, max_mean, max_mean + 1 pA -- the inclusive
    bounds keep and drop the same events as the oracle, and the bounds' own values are kept."""
    from tests.helpers import REGIMES, calib_of
    po = oracle_lib
    cal = REGIMES["identity"]
    rng = np.random.default_rng(12)
    reads, params = [], []
    for lo, hi in ((55, 130), (0, 400)):
        p = capi.default_params(lib)
        p.min_mean, p.max_mean = float(lo), float(hi)
        levels = [lo, hi, hi + 1, 90, 170] + ([lo - 1] if lo > 0 else [])
        vals = rng.choice(levels, 160)
        vals[1:][vals[1:] == vals[:-1]] = 100           # no two equal neighbouring runs
        reads.append(np.repeat(vals, 20).astype(np.int16))
        params.append(p)
    for r, p in zip(reads, params):
        off = np.array([0, r.size], dtype=np.uint64)
        means, moff, info = capi.Mapper(_index(lib, example), params=p, n_slots=1).detect_events(r, off, calib_of([cal]))
        _assert_events_equal(po, means, moff, info, [r], [cal], to_oracle_params(p), "bounds %g..%g" % (p.min_mean, p.max_mean))
        assert np.float32(p.min_mean) in means and np.float32(p.max_mean) in means and means.min() >= p.min_mean and means.max() <= p.max_mean
        assert int(info["total_events"][0]) > int(info["n_events"][0])     # events beyond the bounds were detected and dropped


def zero_pa_signal(cal, rng, n_parts=120):
    """runs of 2 to 15 samples, in turn: exactly 0 pA, one negative level, a mixture of the two, ordinary levels -- stored int16 samples
    for the calibration `cal` (an integer negative offset: the stored value -offset is 0 pA)"""
    z = int(-cal[1])                               # the stored value of 0 pA
    parts = []
    for k in range(n_parts):
        kind = k % 4
        ln = int(rng.integers(2, 16))
        if kind == 0:
            parts.append(np.full(ln, z))
        elif kind == 1:
            parts.append(np.full(ln, int(rng.integers(max(0, z - 40), z))))
        elif kind == 2:
            parts.append(rng.integers(max(0, z - 3), z + 1, ln))
        else:
            parts.append(rng.integers(z + 150, z + 400, ln))
    return np.concatenate(parts).astype(np.int16)


def case_zero_pa_windows(lib, oracle_lib, example):
    """Integer negative offsets: runs of samples at exactly 0 pA, runs of negative pA and mixtures of the two inside one t-statistic
    window (the sums of a window are then exactly zero or of either sign: the exact division's fallback, k_events.hip div_w), between
    ordinary levels; every kept mean and both counters against the oracle, default bounds and none, at several alignments in the batch."""
    from tests.helpers import REGIMES, calib_of
    po = oracle_lib
    rng = np.random.default_rng(13)
    for name in ("promethion", "minion_b"):
        cal = REGIMES[name]
        z = int(-cal[1])
        r = zero_pa_signal(cal, rng)
        for p in (capi.default_params(lib), _wide_bounds(lib)):
            m = capi.Mapper(_index(lib, example), params=p, n_slots=2)
            for pad in (0, 1, 5, 13):
                full = np.concatenate((np.full(pad, z + 300, np.int16), r))
                off = np.array([0, pad, pad + r.size], dtype=np.uint64) if pad else np.array([0, r.size], dtype=np.uint64)
                cals = [REGIMES["minion"], cal] if pad else [cal]
                reads = [full[:pad], r] if pad else [r]
                means, moff, info = m.detect_events(full, off, calib_of(cals))
                _assert_events_equal(po, means, moff, info, reads, cals, to_oracle_params(p), "%s pad %d min_mean %g" % (name, pad, p.min_mean))
        ev = po.detect_events(po.calibrate(r, *cal), to_oracle_params(_wide_bounds(lib)))[0]
        assert (ev["mean"] == 0).any() and (ev["mean"] < 0).any(), name


def per_read_regime_batch(goldens, n_reads, seed=21):
    """golden simulated reads re-digitised, each under a regime of its own, neighbours under different ones -> (raw, offsets, calib, names)"""
    from tests.helpers import REGIMES, calib_of, redigitise
    names = list(REGIMES)
    rng = np.random.default_rng(seed)
    pick = [int(rng.integers(0, len(names)))]
    while len(pick) < n_reads:
        k = int(rng.integers(0, len(names)))
        if k != pick[-1]:
            pick.append(k)
    off_all = goldens["sim_offsets"]
    order = rng.permutation(off_all.size - 1)[:n_reads]
    reads = [redigitise(goldens["sim_signal"][int(off_all[j]):int(off_all[j + 1])], REGIMES["minion"], REGIMES[names[k]]) for j, k in zip(order, pick)]
    off = np.concatenate(([0], np.cumsum([r.size for r in reads]))).astype(np.uint64)
    return np.concatenate(reads), off, calib_of([REGIMES[names[k]] for k in pick]), [names[k] for k in pick]


def case_per_read_calibration_batch(lib, oracle_lib, example, goldens, n_reads=10, device=None):
    """One batch, every read under its own calibration (re-digitised simulated reads), through every batch entry point: unc_map_batch,
    _begin / _end with two mappers in flight, unc_detect_events, UNC_ORDER_T1 and (device: a function that puts the samples in HBM and
    returns their address) the device-resident path -- against the oracle mapping each read under its own calibration."""
    from tests.helpers import calibrate_np
    po = oracle_lib
    raw, off, cal, names = per_read_regime_batch(goldens, n_reads)
    oix = po.Index(example["prefix"])
    want = oracle_hits(oix, raw, off, cal, fresh_mapper_per_read=True)
    share = {n: (int(sum(want["mapped"][i] for i in range(n_reads) if names[i] == n)), names.count(n)) for n in sorted(set(names))}
    assert int(want["mapped"].sum()) >= 0.8 * n_reads, share          # the reads are seeded and mapped, not just left unmapped
    dev_index = _index(lib, example)
    a = capi.Mapper(dev_index, n_slots=4, n_waves=2, slice_events=50)
    assert_hits_equal(a.map_batch(raw, off, cal), want, "per-read calibration, unc_map_batch")
    half = n_reads // 2
    b = capi.Mapper(dev_index, n_slots=3, n_waves=3)
    a.begin_batch(raw, off, cal)
    b.begin_batch(raw[int(off[half]):], (off[half:] - off[half]).astype(np.uint64), cal[half:])
    assert_hits_equal(a.end_batch(), want, "per-read calibration, _begin / _end")
    assert_hits_equal(b.end_batch(), want[half:], "per-read calibration, second half on a second mapper")
    means, moff, info = a.detect_events(raw, off, cal)
    reads = [raw[int(off[i]):int(off[i + 1])] for i in range(n_reads)]
    _assert_events_equal(po, means, moff, info, reads, [tuple(float(c[f]) for f in ("range", "offset", "digitisation")) for c in cal],
                         po.default_params(), "per-read calibration, detect_events")
    t1 = capi.Mapper(dev_index, n_slots=3)
    t1.set_read_order(capi.ORDER_T1)
    assert_hits_equal(t1.map_batch(raw, off, cal), oracle_hits(oix, raw, off, cal, fresh_mapper_per_read=False), "per-read calibration, -t 1 order")
    if device is not None:
        ptr = device(raw)
        assert_hits_equal(a.map_batch_device(ptr, off, cal), want, "per-read calibration, samples in HBM")
        a.begin_batch(ptr, off, cal, on_device=True)
        assert_hits_equal(a.end_batch(), want, "per-read calibration, _begin on device")
    # the calibration reaches the kernels as the numpy restatement says (a sample of every read)
    for i in range(n_reads):
        c = cal[i]
        assert np.array_equal(po.calibrate(reads[i][:64], *(float(c[f]) for f in ("range", "offset", "digitisation"))),
                              calibrate_np(reads[i][:64], c["range"], c["offset"], c["digitisation"]))
    return share


def case_trace_under_another_calibration(lib, oracle_lib, example, goldens):
    """the step-wise trace of the example read re-digitised for a PromethION-like channel"""
    from tests.helpers import REGIMES, calib_of, redigitise
    cal = REGIMES["promethion"]
    raw = redigitise(example["signal"], (example["range"], example["offset"], example["digitisation"]), cal)
    case_trace_matches_oracle_every_event(lib, oracle_lib, example, goldens, raw=raw[:6000], cal=cal)


def case_refused_while_pending(lib, oracle_lib, example, goldens, n_reads=4):
    """unc_detect_events and unc_trace_begin stage into the buffers a batch begun with unc_map_batch_begin is still reading: both are
    refused until unc_map_batch_end, which still returns the oracle's hits; afterwards both work again."""
    from tests.helpers import REGIMES
    raw, off, cal, _ = per_read_regime_batch(goldens, n_reads, seed=22)
    want = oracle_hits(oracle_lib.Index(example["prefix"]), raw, off, cal, fresh_mapper_per_read=True)
    m = capi.Mapper(_index(lib, example), n_slots=2)
    other = np.ascontiguousarray(raw[::-1][:int(off[-1]) // 2])
    m.begin_batch(raw, off, cal)
    with pytest.raises(capi.UncalledHipError):
        m.detect_events(other, np.array([0, 3000, other.size], dtype=np.uint64), capi.make_calib(2, *REGIMES["identity"]))
    with pytest.raises(capi.UncalledHipError):
        next(m.trace(other, capi.make_calib(1, *REGIMES["promethion"])))
    assert_hits_equal(m.end_batch(), want, "batch with refused calls in between")
    means, moff, info = m.detect_events(raw, off, cal)
    assert int(info["n_events"].sum()) == means.size > 0


class _ShuffledRt:
    """stands in for a MapPoolOrd's capi.Realtime: hands each round's chunks over in a random order (the results are put back in the
    caller's), and with `f32` as floats -- calibrated here with the chunk's calibration -- with nonsense in the chunks' calibration,
    which unc_rt_process_chunks_f32 ignores"""

    def __init__(self, rt, po, rng, f32):
        self.rt, self.po, self.rng, self.f32, self.params = rt, po, rng, f32, rt.params
        self.call_sizes, self.mixed_calls = [], 0      # chunks per call; calls that held UNC_RT_FIRST chunks beside continuing ones

    def tap_channel(self, channel):
        return self.rt.tap_channel(channel)

    def close(self):
        self.rt.close()

    def process_chunks(self, chunks, raw):
        first = (chunks["flags"] & capi.RT_FIRST) != 0
        self.call_sizes.append(int(chunks.size))
        self.mixed_calls += int(first.any() and not first.all())
        p = self.rng.permutation(chunks.size)
        ch = chunks[p].copy()
        if self.f32:
            sig = np.zeros(raw.size, dtype=np.float32)
            for c in ch:
                a, n = int(c["offset"]), int(c["n_samples"])
                sig[a:a + n] = self.po.calibrate(raw[a:a + n], float(c["calib"]["range"]), float(c["calib"]["offset"]), float(c["calib"]["digitisation"]))
            ch["calib"]["range"], ch["calib"]["offset"], ch["calib"]["digitisation"] = np.nan, 3.0e38, 0.0
            res = self.rt.process_chunks_f32(ch, sig)
        else:
            res = self.rt.process_chunks(ch, raw)
        out = np.empty_like(res)
        out[p] = res
        return out


def case_chunked_per_channel_calibration(lib, oracle_lib, example, goldens, n_channels=3, reads_per_channel=2, shuffle=False, f32=False,
                                         cut=None, seed=31, params=None, taps=False, min_mapped=0.6, out=None):
    """The chunked path with a calibration per channel AND per read (a channel's successive reads differ: a value kept from the
    channel's first read shows), reads re-digitised for them.  shuffle: every round's chunks in a random order and random channels left
    out of some rounds -- no channel's sequence changes, so a mix-up of the active-chunk index and the channel (descriptors, slot map,
    event-means offsets) shows.  f32: the chunks as floats with nonsense calibrations, which that entry ignores.  Each channel against
    one oracle Mapper fed the same reads in the same order (on the host's threads).  params: other parameters than the defaults (the
    chunk length is chunk_time * sample_rate).  taps: after every finished read the channel's stage tap against the tap its oracle
    Mapper had after the same read.  min_mapped: the share of the reads the oracle must map (reads cut short rarely do).  out: a dict
    that receives every read's RT_RESULT record ("results") and what the calls carried ("call_sizes", "mixed_calls")."""
    from concurrent.futures import ThreadPoolExecutor
    from tests.helpers import REGIMES, redigitise
    from uncalled_amd.realtime import MapPoolOrd
    po = oracle_lib
    dev_index = _index(lib, example)
    oix = po.Index(example["prefix"])
    names = list(REGIMES)
    off = goldens["sim_offsets"]
    n_src = off.size - 1
    reads = {}                                   # key -> (channel, raw, calibration)
    for ch in range(n_channels):
        for j in range(reads_per_channel):
            k = ch * reads_per_channel + j
            base = REGIMES[names[(ch + j) % len(names)]]
            cal = (float(np.float32(base[0] * (1.0 + 1e-4 * (k + 1)))), base[1], base[2])      # every channel and read its own range
            src = goldens["sim_signal"][int(off[k % n_src]):int(off[k % n_src + 1])]
            raw = redigitise(src[:cut] if cut else src, REGIMES["minion"], cal)
            reads[k] = (ch, raw, cal)
    pool = MapPoolOrd(dev_index, n_channels=n_channels, params=params)
    rng = np.random.default_rng(seed)
    pool.rt = _ShuffledRt(pool.rt, po, rng, f32) if (shuffle or f32) else pool.rt
    for k, (ch, raw, cal) in reads.items():
        pool.add_read(ch, k, raw, cal, key=k)
    oracle_taps = {}                              # key -> (tap, ring) of the channel's oracle Mapper after that read

    def oracle_channel(ch):
        om = po.Mapper(oix, to_oracle_params(params) if params is not None else None)
        done = {}
        for k in range(ch * reads_per_channel, (ch + 1) * reads_per_channel):
            _, raw, cal = reads[k]
            h, used = om.chunk_read(po.calibrate(raw, *cal), pool.chunk_len)
            done[k] = (h, used, om.rt_ended())
            if taps:
                oracle_taps[k] = om.rt_tap()
        return done
    import os
    with ThreadPoolExecutor(max_workers=max(1, min(16, len(os.sched_getaffinity(0))))) as ex:
        futs = [ex.submit(oracle_channel, ch) for ch in range(n_channels)]
    want = {}
    for f in futs:
        want.update(f.result())
    got, rounds, skipped = {}, 0, 0
    while pool.running():
        held = {}
        if shuffle:
            busy = [ch for ch, q in enumerate(pool.queues) if q]
            for ch in busy[:-1] if len(busy) > 1 else []:
                if rng.random() < 0.25:
                    held[ch], pool.queues[ch] = pool.queues[ch], []
            skipped += len(held)
        try:
            for key, r in pool.update():
                got[key] = r
                if taps:      # (the channel's next read starts with the next round: this is its state after read `key`)
                    (ta, ra), (tb, rb) = pool.rt.tap_channel(reads[key][0]), oracle_taps[key]
                    assert_rt_taps_equal(ta, ra, tb, rb, "channel %d read %d" % (reads[key][0], key))
        finally:
            for ch, q in held.items():
                pool.queues[ch] = q
        rounds += 1
        assert rounds < 4000
    assert not shuffle or skipped > 0
    if out is not None:
        out["results"] = {k: got[k].tobytes() for k in sorted(got)}
        out["call_sizes"], out["mixed_calls"] = list(getattr(pool.rt, "call_sizes", [])), getattr(pool.rt, "mixed_calls", 0)
    ref_names, dev_names = oix.ref_names(), dev_index.seq_names()
    for k in reads:
        h, (o, used, ended) = got[k]["hit"], want[k]
        assert int(h["status"]) == 0, k
        assert capi.hit_paf_cols(h, dev_names) == po.hit_paf_cols(o, ref_names), k
        for f in ("event_i", "n_nbr", "n_sa", "n_lf", "notes"):
            assert int(h[f]) == int(o[f]), (k, f)
        assert got[k]["state"] == (capi.RT_MAPPED if o["mapped"] else capi.RT_FAILED), k
        assert (pool.chunks_used[k], bool(got[k]["ended"])) == (used, ended), k
    mapped = sum(int(want[k][0]["mapped"]) for k in reads)
    assert mapped >= min_mapped * len(reads), (mapped, len(reads))
    assert all(reads[k][1].size > pool.chunk_len for k in reads) and any(want[k][1] > 1 for k in reads)     # reads of several chunks
    return mapped, len(reads)


# ---- k_rt_events at the edges of a channel's state, and on lanes past 0 (UNC_RT_EVENT_LANES: channels per wavefront)

class _F32Rt:
    """stands in for a MapPoolOrd's capi.Realtime: the reads' samples are floats already and go through unc_rt_process_chunks_f32"""

    def __init__(self, rt):
        self.rt, self.params = rt, rt.params

    def tap_channel(self, channel):
        return self.rt.tap_channel(channel)

    def close(self):
        self.rt.close()

    def process_chunks(self, chunks, sig):
        return self.rt.process_chunks_f32(chunks, np.asarray(sig, dtype=np.float32))


def early_end_reads(goldens, cut=3000):
    """reads of 1, 12, 13, 40, 120, 250 and 400 samples (case_events_edge_cases' steps of five samples plus noise), then an ordinary
    simulated read cut to `cut` samples -> [(int16 samples, calibration)]"""
    rng = np.random.default_rng(17)
    cal = (CAL_RANGE, CAL_OFFSET, CAL_DIGITISATION)
    reads = []
    for ln in (1, 12, 13, 40, 120, 250, 400):
        reads.append((np.repeat(rng.integers(330, 680, ln // 5 + 1), 5)[:ln].astype(np.int16) + rng.integers(-6, 7, ln).astype(np.int16), cal))
    off = goldens["sim_offsets"]
    return reads + [(goldens["sim_signal"][int(off[0]):int(off[1])][:cut], cal)]


def zero_pa_reads(n_parts=400):
    """{regime: (int16 samples, calibration)}: zero_pa_signal of about 400 runs under the two calibrations with an integer negative offset"""
    from tests.helpers import REGIMES
    rng = np.random.default_rng(13)
    return {name: (zero_pa_signal(REGIMES[name], rng, n_parts), REGIMES[name]) for name in ("promethion", "minion_b")}


NOT_NUMBERS = (("nan", np.nan), ("+inf", np.inf), ("-inf", -np.inf))


def not_a_number_reads(oracle_lib, goldens, n=3000, at=1500):
    """{kind: float32 signal}: a simulated read of 3000 samples, calibrated, with one NaN / +inf / -inf at sample 1500; "plain": without"""
    off = goldens["sim_offsets"]
    base = oracle_lib.calibrate(goldens["sim_signal"][int(off[1]):int(off[2])][:n], CAL_RANGE, CAL_OFFSET, CAL_DIGITISATION)
    assert base.size == n
    sigs = {"plain": base}
    for kind, v in NOT_NUMBERS:
        sigs[kind] = base.copy()
        sigs[kind][at] = v
    # finite samples whose windows are not: three of 1.5e19 pA and three of -1.5e19.  Each square (2.25e38) is a float, the sum of two
    # is not, so a window's sum of squares is +inf as a float while the cumulative sums stay finite doubles -- the one operand for which
    # the three-operation division of k_events.hip gives another answer (NaN) than the division it stands for (inf): tstat()'s `bad`
    sigs["huge"] = base.copy()
    sigs["huge"][at:at + 6] = [1.5e19] * 3 + [-1.5e19] * 3
    return sigs


def chunked_reads_against_oracle(lib, oracle_lib, example, params, chunk_len, channels, f32=False, nan_is_nan=False):
    """The chunked path below the PAF on reads given per channel: channels[ch] = the channel's reads in order, each (int16 samples,
    calibration) or a float32 signal (then f32 must be set: the float entry takes the samples as they are; with f32 and int16 reads the
    samples are calibrated here).  After EVERY read the channel's stage tap against its oracle Mapper's after the same read, and
    every result (PAF columns, work counters, notes, state, chunks used, ENDED) against the oracle's.  One Realtime object, closed
    at the end.  -> {(channel, i): (oracle hit, oracle tap)}"""
    from uncalled_amd.realtime import MapPoolOrd
    po = oracle_lib
    dev_index = _index(lib, example)
    oix = po.Index(example["prefix"])
    p = params if params is not None else capi.default_params(lib)
    p.chunk_time = chunk_len / p.sample_rate
    nonsense = (float("nan"), 3.0e38, 0.0)         # the calibration the float entry must ignore
    want = {}
    for ch, reads in enumerate(channels):
        om = po.Mapper(oix, to_oracle_params(p))
        for i, r in enumerate(reads):
            sig = r if isinstance(r, np.ndarray) else po.calibrate(r[0], *r[1])
            assert sig.dtype == np.float32 and (f32 or not isinstance(r, np.ndarray))
            h, used = om.chunk_read(sig, chunk_len)
            want[(ch, i)] = (h, used, om.rt_ended(), om.rt_tap())
    pool = MapPoolOrd(dev_index, n_channels=len(channels), params=p)
    try:
        assert pool.chunk_len == chunk_len
        if f32:
            pool.rt = _F32Rt(pool.rt)
        for ch, reads in enumerate(channels):
            for i, r in enumerate(reads):
                if f32:     # (past add_read, which takes int16: MapPoolOrd cuts and concatenates whatever the queue holds)
                    sig = r if isinstance(r, np.ndarray) else po.calibrate(r[0], *r[1])
                    pool.queues[ch].append((i, sig, nonsense, (ch, i)))
                else:
                    pool.add_read(ch, i, r[0], r[1], key=(ch, i))
        names, ref_names = dev_index.seq_names(), oix.ref_names()
        got, rounds = {}, 0
        while pool.running():
            for key, r in pool.update():
                got[key] = r
                h, (o, used, ended, (tb, rb)) = r["hit"], want[key]
                ta, ra = pool.rt.tap_channel(key[0])
                assert_rt_taps_equal(ta, ra, tb, rb, "channel %d read %d" % key, nan_is_nan=nan_is_nan)
                assert int(h["status"]) == 0, key
                assert capi.hit_paf_cols(h, names) == po.hit_paf_cols(o, ref_names), key
                for f in ("event_i", "n_nbr", "n_sa", "n_lf", "notes"):
                    assert int(h[f]) == int(o[f]), (key, f)
                assert r["state"] == (capi.RT_MAPPED if o["mapped"] else capi.RT_FAILED), key
                assert (pool.chunks_used[key], bool(r["ended"])) == (used, ended), key
            rounds += 1
            assert rounds < 4000
        assert sorted(got) == sorted(want)
    finally:
        pool.rt.close()
    return {k: (v[0], v[3][0]) for k, v in want.items()}


LANES_CHANNELS, LANES_CUT, LANES_CHUNK = 7, 3000, 37


def case_rt_event_lanes(lib, oracle_lib, example, goldens, monkeypatch, lanes, f32):
    """k_rt_events with `lanes` channels per wavefront (UNC_RT_EVENT_LANES, read when the pool is created): seven channels, two reads
    each cut to 3000 samples, chunks of 37 samples, rounds shuffled and thinned -- wavefronts of 3 + 3 + 1 or 2 + 2 + 2 + 1 channels whose
    last one is half full in some rounds and not in others, or one wavefront for all; a channel's second read starts (the new_read
    branch) while its lane neighbours reload their state mid-read; neighbours sit at different phases of the 16-slot ring of sums.
    Every read's stage tap and result against the oracle, and every RT_RESULT record byte for byte against the same reads with one
    channel per wavefront.  What the calls carried is checked, so that the case cannot pass on one lane."""
    p = capi.default_params(lib)
    p.chunk_time = LANES_CHUNK / p.sample_rate
    kw = dict(n_channels=LANES_CHANNELS, reads_per_channel=2, shuffle=True, f32=f32, cut=LANES_CUT, params=p, taps=True, min_mapped=0.0)
    key = ("rt_event_lanes_1", id(lib), f32)
    if key not in _cache:
        monkeypatch.setenv("UNC_RT_EVENT_LANES", "1")
        one = {}
        case_chunked_per_channel_calibration(lib, oracle_lib, example, goldens, out=one, **kw)
        _cache[key] = one["results"]
    monkeypatch.setenv("UNC_RT_EVENT_LANES", str(lanes))
    out = {}
    case_chunked_per_channel_calibration(lib, oracle_lib, example, goldens, out=out, **kw)
    monkeypatch.delenv("UNC_RT_EVENT_LANES")
    assert out["results"] == _cache[key]
    sizes = out["call_sizes"]
    assert max(sizes) >= 2 and len(set(sizes)) > 1, sizes           # several channels in a call, and not always as many
    if lanes == 3:
        assert any(n % 3 for n in sizes) and any(n > 3 and n % 3 == 0 for n in sizes), sizes    # a half-full last wavefront comes and goes
    if lanes == 2:
        assert any(n % 2 for n in sizes) and any(n % 2 == 0 for n in sizes), sizes
    assert out["mixed_calls"] > 0                                    # UNC_RT_FIRST chunks beside continuing ones
    return out


def case_rt_event_lanes_refused(lib, example, monkeypatch):
    """UNC_RT_EVENT_LANES: 1 to 64 or nothing; anything else fails the creation with UNC_ERR_ARG and a message that names the variable"""
    dev_index = _index(lib, example)
    for bad in ("0", "65", "-1", "3x", "two", " "):
        monkeypatch.setenv("UNC_RT_EVENT_LANES", bad)
        with pytest.raises(capi.UncalledHipError, match="UNC_RT_EVENT_LANES"):
            capi.Realtime(dev_index, 1)
    for good in ("", "1", "64"):
        monkeypatch.setenv("UNC_RT_EVENT_LANES", good)
        capi.Realtime(dev_index, 1).close()
    monkeypatch.delenv("UNC_RT_EVENT_LANES")


def case_chunked_reads_that_end_early(lib, oracle_lib, example, goldens, monkeypatch, lanes=None):
    """Reads that end before the profiler's 25-event window fills, or before anything reaches the rolling normaliser (norm.n == 0:
    scale and shift stay 0; the profiler's queue is never popped), one after the other on ONE channel in chunks of 37 samples, then an
    ordinary read that inherits what they left: tap after every read and every result against the oracle.  lanes: channels per
    wavefront (UNC_RT_EVENT_LANES) -- then a second channel runs an ordinary read on the lane beside."""
    reads = early_end_reads(goldens)
    channels = [reads]
    if lanes is not None:
        monkeypatch.setenv("UNC_RT_EVENT_LANES", str(lanes))
        off = goldens["sim_offsets"]
        channels.append([(goldens["sim_signal"][int(off[2]):int(off[3])][:3000], reads[-1][1])])
    try:
        want = chunked_reads_against_oracle(lib, oracle_lib, example, None, 37, channels)
    finally:
        if lanes is not None:
            monkeypatch.delenv("UNC_RT_EVENT_LANES")
    early_end_premises([want[(0, i)][1] for i in range(len(reads))])


def early_end_premises(taps):
    """what the reads of early_end_reads must be for the oracle, or the case tests nothing: taps = the oracle's after each of them"""
    short = taps[:-1]
    assert sum(int(t["prof_n"]) < 25 and int(t["norm_n"]) == 0 for t in short) >= 3, [(int(t["prof_n"]), int(t["norm_n"])) for t in short]
    assert any(int(t["prof_n"]) == 25 for t in short), [int(t["prof_n"]) for t in short]
    assert int(taps[-1]["norm_n"]) > 25, int(taps[-1]["norm_n"])


ZERO_PA_CHUNKED = [(wide, chunk_len, f32) for wide in (False, True) for chunk_len in (37, 4000) for f32 in (False, True)]


def case_chunked_zero_pa_windows(lib, oracle_lib, example, wide, chunk_len, f32):
    """case_zero_pa_windows' signal, lengthened, through the chunked path: t-statistic windows whose sums are exactly zero, negative, or
    of mixed sign send tstat() of k_rt_events to the division itself (`bad` -> tstat_ring<W, false>), as k_events' blocks are sent there.
    Two channels, one per calibration; default mean bounds (most of these events are dropped before the profiler) and none; chunks of
    37 and of 4000 samples; the int16 entry and the float entry.  Taps and results against the oracle."""
    po = oracle_lib
    reads = zero_pa_reads()
    p = _wide_bounds(lib) if wide else capi.default_params(lib)
    want = chunked_reads_against_oracle(lib, po, example, p, chunk_len, [[reads[name]] for name in reads], f32=f32)
    for ch, name in enumerate(reads):
        raw, cal = reads[name]
        zero_pa_premises(po, lib, raw, cal, name)
        tap = want[(ch, 0)][1]
        if not wide:       # events were detected and dropped for their means before the profiler saw them
            assert int(tap["det_total_events"]) > int(tap["norm_n"]) + 25, (name, int(tap["det_total_events"]), int(tap["norm_n"]))


def zero_pa_premises(po, lib, raw, cal, name):
    ev = po.detect_events(po.calibrate(raw, *cal), to_oracle_params(_wide_bounds(lib)))[0]
    assert (ev["mean"] == 0).any() and (ev["mean"] < 0).any(), name


def case_chunked_samples_that_are_no_numbers(lib, oracle_lib, example, goldens):
    """The float entry takes samples as they are: one NaN, +inf or -inf at sample 1500 of a 3000-sample read in chunks of 400 -- the
    sums of the detector's ring are no numbers from there on (inf - inf for the infinities), no t-statistic compares true, no event
    closes, and the read, which maps within 2000 samples when it is left alone, is given all its chunks and fails.  Each kind first on
    a fresh channel (channels 0 to 2), where a plain read follows and starts from the state the poisoned one left, and behind a read
    that mapped (channels 3 to 5).  Channels 6 and 7: the same with six finite samples of +-1.5e19 pA, whose windows' sums of squares
    are infinite as floats (not_a_number_reads).  Taps and results against the oracle; NaN against NaN where both hold one."""
    sigs = not_a_number_reads(oracle_lib, goldens)
    channels = [[sigs[kind], sigs["plain"]] for kind, _ in NOT_NUMBERS] + [[sigs["plain"], sigs[kind]] for kind, _ in NOT_NUMBERS]
    channels += [[sigs["huge"], sigs["plain"]], [sigs["plain"], sigs["huge"]]]
    want = chunked_reads_against_oracle(lib, oracle_lib, example, None, 400, channels, f32=True, nan_is_nan=True)
    plain = want[(3, 0)][1]
    for ch in range(3):        # the poisoned read went on to its end (8 chunks' samples), and closed fewer events than the plain one
        tap = want[(ch, 0)][1]
        assert int(tap["det_t"]) == 3001 and int(tap["det_total_events"]) < int(plain["det_total_events"]), (ch, tap)


def ring_wrap_reads(goldens):
    """[(int16 samples, calibration)]: zero_pa_signal of 5200 runs -- under mean bounds that drop nothing more than 6000 of its events
    reach the rolling normaliser, whose ring of 6000 wraps -- and behind it the reads of early_end_reads"""
    from tests.helpers import REGIMES
    cal = REGIMES["promethion"]
    return [(zero_pa_signal(cal, np.random.default_rng(19), 5200), cal)] + early_end_reads(goldens)


def ring_wrap_premises(taps):
    """the oracle's taps after the reads of ring_wrap_reads: the ring is full and has wrapped after the first, and stays where it is
    through the reads that push nothing"""
    assert int(taps[0]["norm_n"]) == 6000 and int(taps[0]["det_total_events"]) > 6500 and 0 < int(taps[0]["norm_wr"]) < 3000, taps[0]
    assert sum(int(t["norm_wr"]) == int(taps[0]["norm_wr"]) for t in taps[1:]) >= 3, [int(t["norm_wr"]) for t in taps]


def case_chunked_ring_wraps_then_short_reads(lib, oracle_lib, example, goldens):
    """One read that pushes more events than the rolling normaliser's ring holds (the write position passes the place the read pointer
    was left at: roll_skip_unread at every chunk's start is what keeps the ring from counting as full), through the float entry in
    chunks of 4000 samples; then the reads that end early, whose scale and shift come from a full ring they add nothing to."""
    want = chunked_reads_against_oracle(lib, oracle_lib, example, _wide_bounds(lib), 4000, [ring_wrap_reads(goldens)], f32=True)
    ring_wrap_premises([want[k][1] for k in sorted(want)])


# ---------------------------------------------------------------- the FM layer (fm_dev.h, k_taps.hip) against tests/fm_naive.py
# Tiny references whose rows end, and whose primary row falls, at every edge of the 64-symbol blocks of the 32-bit rank table and the
# 128-symbol blocks of the BWA layout; each is loaded as k_map meets it (32-bit table, dense SA), on the BWA-sampled SA, and without
# the 32-bit table (the 64-bit arithmetic of the references of 2^32 rows and more).
FM_RANDOM_LPAC = (1, 2, 3, 5, 16, 31, 32, 33, 63, 64, 65, 96, 127, 128, 129)
FM_PRIMARY_SEEDS = {291: 1, 51: 63, 198: 64, 75: 65, 146: 127, 13: 128}       # default_rng(seed).integers(0, 4, 64) -> the primary row
FM_DEGENERATE = ("allA", "period2", "period2rc", "unit21")
FM_SELF_ALIGN = ("random-33", "random-64", "random-129", "contigs")
FM_LOADS = (("default", {}), ("bwa_sa", {"UNC_DENSE_SA": "0"}), ("no_fm32", {"UNC_FM32": "0"}))
FM_REFERENCES = tuple("random-%d" % n for n in FM_RANDOM_LPAC) + tuple("primary-%d" % s for s in FM_PRIMARY_SEEDS) + FM_DEGENERATE + ("contigs",)
_fm_cache = {}


def fm_reference_codes(name):
    """-> (codes, contig lengths or None)"""
    kind, _, arg = name.partition("-")
    if kind == "random":
        return np.random.default_rng(0).integers(0, 4, int(arg)).astype(np.uint8), None
    if kind == "primary":
        return np.random.default_rng(int(arg)).integers(0, 4, 64).astype(np.uint8), None
    if kind == "allA":
        return np.zeros(64, dtype=np.uint8), None                               # the text is A^64 T^64
    if kind == "period2":
        return np.tile(np.array([0, 1], dtype=np.uint8), 32), None              # (AC)^32 (GT)^32
    if kind == "period2rc":
        return np.tile(np.array([0, 3], dtype=np.uint8), 32), None              # (AT)^64: its own reverse complement
    if kind == "unit21":
        return np.tile(np.random.default_rng(21).integers(0, 4, 21).astype(np.uint8), 4)[:64], None
    if kind == "contigs":
        return np.random.default_rng(7).integers(0, 4, 1000).astype(np.uint8), [300, 700]
    raise KeyError(name)


def fm_reference(name, tmp_path):
    """the index files of a reference under tmp_path -> (prefix, its NaiveFM with the k-mer ranges and trajectories worked out once)"""
    from tests import fm_naive
    codes, lens = fm_reference_codes(name)
    prefix = tmp_path / name
    if name not in _fm_cache:
        fm = fm_naive.build(prefix, codes, lens)
        fm.kr = fm.kmer_ranges()
        fm.traj = fm.self_align() if name in FM_SELF_ALIGN else None
        _fm_cache[name] = fm
    else:
        from uncalled_amd.build_index import build_from_codes
        lens = lens or [codes.size]
        build_from_codes(prefix, ["c%d" % i for i in range(len(lens))], [""] * len(lens), lens, codes)
    return prefix, _fm_cache[name]


def _first_diff(got_s, got_e, want_s, want_e, s, e, c):
    bad = np.flatnonzero((got_s != want_s) | (got_e != want_e))
    if bad.size == 0:
        return None
    i = int(bad[0])
    return "%d of %d steps differ; the first: get_neighbor(%d, %d, %d) = (%d, %d), naive (%d, %d)" % (
        bad.size, s.size, s[i], e[i], c[i], got_s[i], got_e[i], want_s[i], want_e[i])


def fm_queries(fm):
    """(s, e, c) of the backward steps asked of a reference.  Up to 258 rows: every range 1 <= s <= e <= seq_len with every base,
    and every INVERTED pair e + 1 < s <= seq_len + 1 -- no path holds one, but fm_nbr_issue guards its shared-block load against them
    (`kk <= ll`) and the tap answers them with the two plain ranks.  The 2 000-row reference: every single-row range and 20 000 random ones, with e == seq_len, s - 1 == primary and e == primary among them."""
    n = fm.n
    if n <= 258:
        i, j = np.triu_indices(n)                       # i <= j
        s, e = i + 1, j + 1
        i2, j2 = np.triu_indices(n, 1)                  # i2 < j2: e = i2 + 1, s = j2 + 2  (e + 1 < s <= n + 1)
        s, e = np.concatenate((s, j2 + 2)), np.concatenate((e, i2 + 1))
    else:
        rng = np.random.default_rng(n)
        m = 20000
        rs = rng.integers(1, n + 1, m)
        re = np.minimum(n, rs + np.where(rng.integers(0, 2, m) == 0, rng.integers(0, 70, m), rng.integers(0, n, m)))
        re[:2000] = n                                                       # e == seq_len
        rs[2000:3000] = fm.primary + 1                                      # s - 1 == primary
        re[2000:3000] = np.minimum(n, fm.primary + 1 + rng.integers(0, 300, 1000))
        re[3000:4000] = fm.primary                                          # e == primary
        rs[3000:4000] = np.maximum(1, fm.primary - rng.integers(0, 300, 1000))
        rows = np.arange(1, n + 1)
        s, e = np.concatenate((rows, rs)), np.concatenate((rows, re))
    s, e = np.repeat(s, 4), np.repeat(e, 4)
    c = np.tile(np.arange(4), s.size // 4)
    return s.astype(np.uint64), e.astype(np.uint64), c.astype(np.uint8)


def case_fm_tiny(lib, oracle_lib, tmp_path, monkeypatch, name):
    prefix, fm = fm_reference(name, tmp_path)
    n = fm.n
    kind, _, arg = name.partition("-")
    if kind == "primary":
        assert (n, fm.primary) == (128, FM_PRIMARY_SEEDS[int(arg)]), (name, fm.primary)
    s, e, c = fm_queries(fm)
    want_s, want_e = fm.get_neighbors(s, e, c)
    rows = np.arange(n + 1, dtype=np.uint64)
    want_sa = fm.sa_rows()
    # the oracle on the same files: the naive module is not wrong the way the device is
    oix = oracle_lib.Index(prefix)
    assert int(oix.size) == n
    assert np.array_equal(oix.kmer_ranges(), fm.kr), name
    legal = np.flatnonzero(s <= e)
    for i in legal[:: max(1, legal.size // 300)]:
        assert oix.get_neighbor(int(s[i]), int(e[i]), int(c[i])) == (int(want_s[i]), int(want_e[i])), (name, s[i], e[i], c[i])
    for r in range(0, n + 1, max(1, n // 300)):
        assert oix.sa(r) == int(want_sa[r]), (name, r)
    sizes = {}
    for what, env in FM_LOADS:
        for k in ("UNC_DENSE_SA", "UNC_FM32"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        ix = capi.Index(prefix, lib=lib)
        sizes[what] = ix.device_bytes()
        assert ix.size == n
        got_s, got_e = ix.get_neighbor(s, e, c)
        assert _first_diff(got_s, got_e, want_s, want_e, s, e, c) is None, (name, what, _first_diff(got_s, got_e, want_s, want_e, s, e, c))
        got_sa = ix.sa(rows)
        bad = np.flatnonzero(got_sa != want_sa)
        assert bad.size == 0, (name, what, "sa(%d) = %d, naive %d" % (bad[0], got_sa[bad[0]], want_sa[bad[0]]))
        kr = ix.kmer_ranges()
        bad = np.flatnonzero((kr != fm.kr).any(axis=1))
        assert bad.size == 0, (name, what, "k-mer %d: %s, naive %s" % (bad[0], kr[bad[0]], fm.kr[bad[0]]))
        if fm.traj is not None:
            lens, full_len = ix.self_align(prefix, 1, cap=64)
            assert [int(x) for x in full_len] == [len(t) for t in fm.traj], (name, what)
            for i, t in enumerate(fm.traj):
                assert [int(x) for x in lens[i, :min(64, len(t))]] == t[:64] and not lens[i, len(t):].any(), (name, what, i)
        ix.close()
    # the knobs did what they say: the dense table / the 32-bit table are what the two other loads leave out
    assert sizes["default"] - sizes["bwa_sa"] == ((n + 2) // 2) * 12 + 16, sizes
    assert sizes["default"] - sizes["no_fm32"] == ((n + 63) // 64 + 1) * 32, sizes


# ---------------------------------------------------------------- the suffix sort (k_sort.hip) at its edges
SA_EDGE_LENGTHS = (1, 2, 20, 21, 22, 41, 42, 43, 63, 64, 65, 2047, 2048, 2049, 4097)


def sa_edge_texts(n):
    """texts of n symbols around the 21-symbol first key: (name, codes)"""
    rng = np.random.default_rng(1000 + n)
    yield "random", rng.integers(0, 4, n).astype(np.uint8)
    yield "zeros", np.zeros(n, dtype=np.uint8)                              # ties run to the end of the text: doubling until k > n / 2
    yield "period2", (np.arange(n) & 1).astype(np.uint8)
    yield "unit21", np.tile(rng.integers(0, 4, 21).astype(np.uint8), n // 21 + 1)[:n]      # ties exactly one first key wide
    t = rng.integers(0, 4, n).astype(np.uint8)
    t[-30:] = 0                                                             # symbol 0 against the past-the-end marker of the first key
    yield "zero_tail", t


def case_suffix_sort_edges(lib):
    from uncalled_amd.build_index import suffix_array
    for n in SA_EDGE_LENGTHS:
        for name, t in sa_edge_texts(n):
            s = bytes(t + 1)
            naive = np.array(sorted(range(n), key=lambda i: s[i:]), dtype=np.int64)
            got = capi.build_suffix_array(t, 0, lib)
            assert np.array_equal(got, naive), (n, name)
            assert np.array_equal(suffix_array(t), naive), (n, name)


def case_radix_sort_edges(lib):
    """unc_sort_pairs_u64 on the inputs a random draw does not give: one key, two values per digit, sorted and reversed keys, a top
    digit that is partly used -- around the 2 048-pair tile, values given and generated."""
    rng = np.random.default_rng(2)
    for n in (65, 2047, 4096, 4097):
        two = np.where(rng.integers(0, 2, n) == 0, np.uint64(0x01FE01FE01FE01FE), np.uint64(0xFE01FE01FE01FE01))
        inputs = [("equal", np.full(n, 0x0123456789ABCDEF, dtype=np.uint64), 64),
                  ("two_values", two, 64), ("two_values_low_byte", two & np.uint64(0xFF), 8),
                  ("ascending", np.arange(n, dtype=np.uint64), 16), ("descending", np.arange(n, dtype=np.uint64)[::-1].copy(), 16),
                  ("bits9", rng.integers(0, 1 << 9, n, dtype=np.uint64), 9), ("bits17", rng.integers(0, 1 << 17, n, dtype=np.uint64), 17)]
        for name, keys, bits in inputs:
            want = np.argsort(keys, kind="stable").astype(np.uint64)
            sk, perm = capi.sort_pairs(keys, None, bits, lib=lib)
            assert np.array_equal(perm, want) and np.array_equal(sk, keys[want]), (n, name, "iota")
            vals = rng.integers(0, 2 ** 63, size=n, dtype=np.uint64)
            sk2, sv = capi.sort_pairs(keys, vals, bits, lib=lib)
            assert np.array_equal(sk2, keys[want]) and np.array_equal(sv, vals[want]), (n, name, "values")


# ---------------------------------------------------------------- unc_match_probs beyond one read's levels
def case_match_probs_levels(lib, oracle_lib, example):
    """PoreModel::match_prob of all 1 024 k-mers (k_match_probs) for levels over the whole range of a normalised read, every model mean
    itself (a difference of exactly zero) and the values a float can take at its ends -- bit for bit what the oracle gives, NaN where it
    gives NaN."""
    dev_index = _index(lib, example)
    rng = np.random.default_rng(5)
    means = np.asarray(oracle_lib.model_tables()[0], dtype=np.float32)
    special = np.array([0.0, -0.0, 1e-40, 1e30, -1e30, np.inf, -np.inf, np.nan], dtype=np.float32)
    levels = np.concatenate((rng.uniform(40.0, 140.0, 1000).astype(np.float32), means, special))
    assert levels.size == 2032 and np.signbit(special[1]) and 0 < special[2] < np.finfo(np.float32).tiny
    got = dev_index.match_probs(levels)
    want = np.stack([oracle_lib.match_probs(lv) for lv in levels])
    nan = np.isnan(want)
    assert nan[-1].all() and not nan[:-3].any()      # (NaN in, NaN out; no finite level gives one)
    assert np.array_equal(np.isnan(got), nan)
    bad = np.argwhere((got.view(np.uint32) != want.view(np.uint32)) & ~nan)
    assert bad.size == 0, "%d differ; level %r, k-mer %d: %r, oracle %r" % (
        len(bad), levels[bad[0][0]], bad[0][1], got[tuple(bad[0])], want[tuple(bad[0])])


# ---------------------------------------------------------------- what the creations allocate, by name
# unc_*_device_bytes and the geometry of creations whose every size is named (no size taken from the free memory): the values of
# e40587f (the commit before the creations became plan / allocations / builds) under the emulator; the emulator and the MI355X both give them
CREATION_INDEX_BYTES = dict(default=173932, bwa_sa=53904, no_fm32=163884)
CREATION_MAPPERS = (
    (dict(n_slots=2, n_waves=2, pool_chunks=16), 7946240,
     dict(n_waves=2, n_slots=2, slice_events=0, pool_chunks=16, max_clusters=1 << 20)),
    (dict(n_slots=64, n_waves=2, pool_chunks=16, sched_parts=1), 156751488,
     dict(n_waves=2, n_slots=64, slice_events=1024, pool_chunks=16, max_clusters=1 << 20)),
    (dict(n_slots=3, n_waves=2, pool_chunks=16, max_clusters=4096, max_seed_paths=512), 8944512,
     dict(n_waves=2, n_slots=3, slice_events=1024, pool_chunks=16, max_clusters=4096)),
)
CREATION_RT_BYTES = 15008436      # one channel, UNC_RT_POOL_CHUNKS=64


def case_creation_sizes(lib, example, monkeypatch):
    for k in ("UNC_DENSE_SA", "UNC_FM32", "UNC_WIDE_KEYS", "UNC_BUCKET_SHIFT", "UNC_RT_POOL_CHUNKS"):
        monkeypatch.delenv(k, raising=False)
    got = {}
    for what, env in FM_LOADS:
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        ix = capi.Index(example["prefix"], lib=lib)
        got[what] = ix.device_bytes()
        ix.close()
        for k in env:
            monkeypatch.delenv(k)
    print("index device_bytes:", got)
    assert got == CREATION_INDEX_BYTES
    dev_index = _index(lib, example)
    for kw, want_bytes, want_geometry in CREATION_MAPPERS:
        m = capi.Mapper(dev_index, **kw)
        print("mapper", kw, m.device_bytes(), m.geometry())
        assert (m.device_bytes(), m.geometry()) == (want_bytes, want_geometry), kw
        m.close()
    monkeypatch.setenv("UNC_RT_POOL_CHUNKS", "64")
    rt = capi.Realtime(dev_index, n_channels=1)
    print("realtime device_bytes:", rt.device_bytes())
    assert rt.device_bytes() == CREATION_RT_BYTES
    rt.close()
