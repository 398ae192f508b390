"""GPU: the adaptive-band DTW with an open end on the gfx950 library against the checker (tests/dtw_adapt_check.c, anchored by
tests/test_dtw_adapt_cpu.py): the emulator file's cases -- the shapes, the band's width edges at B = 64, 128 and 256 (rows around
B / 2, B and above; sweeps that end early at every residue of the flushes; non-finite events at the first and the last column; path
lengths around 64 with two and four cells a lane), the adaptive band through a custom model, the training accumulator, the pile-up,
the rounds, the other options and a path without a start (tests/adapt_pipeline_cases.py) -- then what only a GPU holds: more
alignments than the launch has wavefronts (small ones, and the edge shapes whose bands moved), anti-diagonal indices past 2^16 with
linear memory, two threads, the host module, the command line.  Everything runs in this one process; each of the two command-line
tests (`dtw --adaptive`, `train --adaptive`) starts one child and waits for it."""
import subprocess
import sys

import numpy as np
import pytest

import adapt_pipeline_cases as apc
import align_cases as ac
import dtw_adapt_cases as xc
import dtw_cases as dc
from conftest import EX_PREFIX, GOLD, ROOT
from dtw_adapt_check import LEFT_BAND, OK, REF_END, AdaptChecker, adapt_crumb_bytes

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def checker():
    return AdaptChecker()


@pytest.fixture(scope="module")
def means(checker):
    return checker.model[:1024]


# ------------------------------------------------------------------ 1. the emulator file's cases
@pytest.mark.parametrize("cost,weights", [(c, w) for c in (xc.R94P, xc.R94D) for w in xc.WEIGHT_SETS])
def test_shapes_equal_the_checker(hip_lib, checker, means, cost, weights):
    seen = set()
    for b in xc.shape_batches(means, cost, weights):
        _, _, want = xc.check(checker, b)
        seen |= {w["status"] for w in want}
    assert seen == {OK, REF_END}
    ev, km = xc.case_of_path_len(checker, means, 128, cost, weights)
    xc.check(checker, xc.batch("a path of 128 pairs", [ev], [km], cost, weights, 64))


def test_a_band_that_binds(hip_lib, checker, means):
    xc.check_binding(checker, means)


def test_events_that_are_no_numbers_and_ties(hip_lib, checker, means):
    _, _, want = xc.check(checker, xc.nonfinite_batch(means))
    assert want[0]["status"] == LEFT_BAND
    for cost, weights in ((xc.R94P, (2.0, 1.0, 100.0)), (xc.R94P, (0.0, 0.0, 0.0)), (xc.R94D, (0.0, 0.0, 0.0))):
        xc.check(checker, xc.nonfinite_batch(means, cost=cost, weights=weights))
    b = xc.all_equal_batch(means)
    xc.check(checker, b)
    xc.check(checker, xc.batch("all ties", b["evs"], b["kms"], xc.R94P, (0.0, 0.0, 0.0), 128))


def test_interface(hip_lib, checker, means):
    xc.check_argument_errors(hip_lib)
    xc.check_caller_offsets(hip_lib, checker, means)
    xc.check_rounds_and_too_large(checker, means)


def test_align_pipeline_on_the_example_read(hip_lib, checker):
    import pileup_cases as pc
    xc.check_pipeline(ac.Goldens(), pc.Ctx(hip_lib, EX_PREFIX), checker)


@pytest.mark.parametrize("B", [64, 128, 256])
def test_band_edges(hip_lib, checker, means, B):
    xc.check_edges(checker, means, B)


@pytest.mark.parametrize("B", [64, 128, 256])
def test_early_end_of_the_sweep(hip_lib, checker, means, B):
    xc.check_early_end(checker, means, B)


def test_non_finite_events_at_the_first_and_last_column(hip_lib, checker, means):
    xc.check_nonfinite_ends(checker, means)


@pytest.mark.parametrize("B", [128, 256])
def test_path_length_residues_with_several_cells_a_lane(hip_lib, checker, means, B):
    xc.check_path_residues(checker, means, B)


def test_the_host_module_takes_the_keyword(hip_lib, checker, means):
    from uncalled_amd import _uncalled_amd as unc
    ev, km = xc.follow_case(np.random.default_rng(61), means, 150, 160)
    prm = unc.DTWParams(0, 1.0, 1.0, 1.0)
    for cls, cost in ((unc.DTWr94d, xc.R94D), (unc.DTWr94p, xc.R94P)):
        want = checker.dtw(ev, km, cost, 1.0, 1.0, 1.0, 128)
        assert want["status"] == OK
        d = cls(ev.tolist(), km.tolist(), prm, adaptive=128)
        assert xc.same_float(d.score(), want["score"]) and [tuple(p) for p in d.get_path()] == [tuple(map(int, p)) for p in want["path"]]
        assert d.status() == OK and cls(ev.tolist(), km.tolist(), prm).get_path()[0] == (ev.size - 1, km.size - 1)
    with pytest.raises(RuntimeError):
        unc.DTWr94d(ev.tolist(), km.tolist(), prm, adaptive=96)


# ------------------------------------------------------------------ 1b. the adaptive band through model, training, pile-up and options
@pytest.fixture(scope="module")
def pipe(hip_lib):
    return apc.Ctx(hip_lib, EX_PREFIX)


def test_pipeline_with_a_custom_model(pipe):
    apc.check_custom_model(pipe)


@pytest.mark.parametrize("keep_shared", [False, True])
def test_training_with_an_open_end(pipe, keep_shared):
    apc.check_training(pipe, keep_shared)


def test_pipeline_rounds_through_the_hook(pipe):
    apc.check_rounds(pipe)


def test_pipeline_options_with_the_adaptive_band(pipe):
    apc.check_options(pipe)


def test_a_path_without_a_start_in_the_pipeline(pipe):
    apc.check_left_band(pipe)


# ------------------------------------------------------------------ 2. more alignments than wavefronts
def test_more_alignments_than_wavefronts(hip_lib, checker, means):
    """three times more alignments than the launch has wavefronts (16 per compute unit), cycling 50 small cases: a wavefront goes
    round the queue loop again with the band's state of its previous alignment left over"""
    import torch
    from uncalled_amd import capi
    n = 3 * 16 * torch.cuda.get_device_properties(0).multi_processor_count + 7
    q = dc.queue_batches(means, n, 50, 40)[0]
    distinct = {}
    for a, d in enumerate(q["of"]):
        distinct.setdefault(d, a)
    for B in (64, 256):
        done = {d: checker.dtw(q["evs"][a], q["kms"][a], xc.R94D, 2.0, 1.0, 100.0, B) for d, a in distinct.items()}
        b = xc.batch(f"queue B {B}", q["evs"], q["kms"], xc.R94D, (2.0, 1.0, 100.0), B)
        res, paths = xc.run(b)
        assert capi.dtw_last_timing()[1] == 1
        xc.assert_equal_to_checker(res, paths, [done[d] for d in q["of"]], b["name"])


def test_more_alignments_than_wavefronts_with_bands_that_moved(hip_lib, checker, means):
    """the same queue cycling the 42 edge alignments at B = 128 and 256: a wavefront goes round the loop again with the rows, model
    values and events of a band that moved left over in its registers"""
    import torch
    from uncalled_amd import capi
    n = 3 * 16 * torch.cuda.get_device_properties(0).multi_processor_count + 7
    for B in (128, 256):
        e = xc.edge_batches(means, xc.R94D, (1.0, 1.0, 1.0), B)[0]
        done = xc.wanted(checker, e)
        assert len(done) == 42 and any(w["lo"].max() > -B // 2 + 16 for w in done)
        of = [a % 42 for a in range(n)]
        b = xc.batch(f"queue of edges B {B}", [e["evs"][d] for d in of], [e["kms"][d] for d in of], e["cost"], e["weights"], B)
        res, paths = xc.run(b)
        assert capi.dtw_last_timing()[1] == 1
        xc.assert_equal_to_checker(res, paths, [done[d] for d in of], b["name"])


# ------------------------------------------------------------------ 3. anti-diagonal indices past 2^16, linear memory
def test_a_long_alignment_in_linear_memory(hip_lib, checker, means):
    from uncalled_amd import capi
    rows, cols, B = 40000, 45000, 64
    rng = np.random.default_rng(62)
    km = rng.integers(0, 1024, rows).astype(np.uint16)
    ev = dc.follow(rng, means, km[:30000], cols)
    _, paths, want = xc.check(checker, xc.batch("long", [ev], [km], xc.R94D, (1.0, 1.0, 1.0), B))
    ms, rounds, held = capi.dtw_last_timing()
    print(f"40000 x 45000 at B = 64: kernel {ms:.2f} ms, {held} bytes of back-pointers, path of {want[0]['path_len']}, status {want[0]['status']}")
    assert want[0]["lo"].size > 65536 and want[0]["path_len"] >= cols and rounds == 1
    assert held == adapt_crumb_bytes(rows, cols, B) and held < dc.crumb_bytes(rows, cols) / 100


# ------------------------------------------------------------------ 4. two threads
def test_two_threads_each_on_a_stream_of_its_own(hip_lib, checker, means):
    import threading

    import torch
    from uncalled_amd import capi
    b = xc.rounds_batch(means)
    want = xc.wanted(checker, b)
    xc.run(b)       # (the model's upload, not raced here)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    barrier = threading.Barrier(2, timeout=60)
    out = [None, None]

    def work(t, ws):
        try:
            barrier.wait()
            res, paths = xc.run(b, workspace_bytes=ws, stream=streams[t].cuda_stream)
            out[t] = (res, paths, capi.dtw_last_timing())
        except BaseException as e:      # (reported by the asserts below)
            out[t] = e

    threads = [threading.Thread(target=work, args=(0, b["workspace"])), threading.Thread(target=work, args=(1, 0))]
    for th in threads:
        th.start()
    for th in threads:
        th.join(timeout=120)
    for t in range(2):
        assert isinstance(out[t], tuple), out[t]
        xc.assert_equal_to_checker(out[t][0], out[t][1], want, f"thread {t}")
    assert out[0][2][1] >= 3 and out[0][2][2] <= b["workspace"] and out[1][2][1] == 1 and out[1][2][2] == sum(b["sizes"])


# ------------------------------------------------------------------ 5. the command line, once, in one child process
def test_the_cli_aligns_a_whole_read_from_its_hit(hip_lib, checker, tmp_path):
    """the example read mapped here through capi, its PAF line fed to `python -m uncalled_amd dtw --paf --adaptive 128` in a child
    process (waited for): the path file and the mean score equal capi.align_ref_batch with the same query, stretch and options"""
    import math
    from uncalled_amd import capi
    ex = np.load(GOLD / "example_read.npz")
    rid = str(ex["read_id"])
    ix = capi.Index(EX_PREFIX)
    raw = ex["signal"]
    offsets = np.array([0, raw.size], np.uint64)
    calib = capi.make_calib(1, float(ex["range"]), float(ex["offset"]), float(ex["digitisation"]))
    hit = capi.Mapper(ix, n_slots=64).map_batch(raw, offsets, calib)[0]
    cols = capi.hit_paf_cols(hit, ix.seq_names())
    assert cols[1] != "*", cols
    f = [rid] + [str(c) for c in cols]          # the PAF line's columns 1 to 12
    paf = tmp_path / "hit.paf"
    paf.write_text("\t".join(f) + "\n")
    prefix = str(tmp_path / "out_")
    cmd = [sys.executable, "-m", "uncalled_amd", "dtw", str(EX_PREFIX), str(GOLD / "example_read.fast5"), str(paf), "--paf", "--adaptive", "128",
           "-o", prefix, "--max-events", "0"]
    run = subprocess.run(cmd, cwd=str(ROOT), capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    # the same query here: from the hit's first sample to the read's end, the stretch from the hit's start on its strand
    prm = capi.default_params()
    fwd, ref_st, ref_en = f[4] == "+", int(f[7]), int(f[8])
    smp_st = int(f[2]) * 80 // 9
    n = max(5, math.ceil((raw.size - smp_st) * float(prm.bp_per_sec) / float(prm.sample_rate) * 1.5))
    stretch = (0, ref_st, min(ref_st + n, int(ix.seq_len(0))), True) if fwd else (0, max(ref_en - n, 0), ref_en, False)
    res, levs, paths, kms = capi.align_ref_batch(capi.RefSeq(ix, EX_PREFIX), raw, offsets, calib, [(0, smp_st, raw.size)], [stretch],
                                                 capi.align_opts(max_events=0, adaptive=128), levels=True, paths=True, kmers=True)
    st = int(res["status"][0])
    assert st in (OK, REF_END), st
    w = checker.dtw(levs[0], kms[0], xc.R94D, 1.0, 1.0, 1.0, 128)
    assert w["status"] == st and np.array_equal(paths[0], w["path"]) and xc.same_float(res["dtw"]["score"][0], w["score"])
    fields = run.stdout.strip().split("\n")
    assert len(fields) == 1, run.stdout
    f = fields[0].split("\t")
    assert f[:2] == [rid, "%.6g" % float(res[0]["dtw"]["mean_score"])] and (f[3:] == ["status 7"] if st == REF_END else len(f) == 3), f
    rows = [ln.split("\t") for ln in open(prefix + rid + ".txt").read().strip().split("\n")]
    assert [(int(r[0]), int(r[1])) for r in rows] == [tuple(map(int, p)) for p in paths[0][::-1]]


def test_the_cli_trains_with_the_adaptive_band(hip_lib, tmp_path):
    """the same PAF line fed to `python -m uncalled_amd train --adaptive 128 --iters 2 --min-obs 2 --max-events 2000` in one child
    process (waited for): the saved model equals the same two iterations driven through capi on the query and stretch that
    extend_paf_queries makes.  With --adaptive the query is the read from the hit to its END, some 5000 columns of the example read:
    --max-events 2000 skips it (UNC_ALIGN_TOO_MANY) on both sides and the model stays the prior.  So the iterations behind the command
    (train_model) run once more in this process without the limit, where the read is aligned and the model moves."""
    from uncalled_amd import __main__ as cli
    from uncalled_amd import _uncalled_amd as unc
    from uncalled_amd import capi
    ex = np.load(GOLD / "example_read.npz")
    ix = capi.Index(EX_PREFIX)
    raw = ex["signal"]
    offsets = np.array([0, raw.size], np.uint64)
    calib = capi.make_calib(1, float(ex["range"]), float(ex["offset"]), float(ex["digitisation"]))
    hit = capi.Mapper(ix, n_slots=64).map_batch(raw, offsets, calib)[0]
    cols = capi.hit_paf_cols(hit, ix.seq_names())
    assert cols[1] != "*", cols
    paf = tmp_path / "hit.paf"
    paf.write_text("\t".join([str(ex["read_id"])] + [str(c) for c in cols]) + "\n")
    out = tmp_path / "trained.txt"
    cmd = [sys.executable, "-m", "uncalled_amd", "train", str(EX_PREFIX), str(GOLD / "example_read.fast5"), str(paf), "-o", str(out), "--adaptive", "128",
           "--iters", "2", "--min-obs", "2", "--max-events", "2000"]
    run = subprocess.run(cmd, cwd=str(ROOT), capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    rows = [ln for ln in run.stderr.split("\n") if ln.startswith("iteration ")]
    assert len(rows) == 2
    got = capi.Model.load(out)

    queries = cli.load_paf_queries(str(paf))
    rd = cli.load_query_reads(unc, str(GOLD / "example_read.fast5"), queries)
    cli.clip_paf_queries(queries, rd)
    cli.extend_paf_queries(queries, rd, ix)
    assert len(rd) == 1
    rid, samples, cal = rd[0]
    q = queries[rid]
    assert q["smp_en"] == len(samples) == raw.size
    calib1 = capi.make_calib(1, 0, 0, 1)
    calib1[0] = cal
    stretch = [(ix.seq_names().index(q["ref"]), q["ref_st"], q["ref_en"], q["fwd"])]
    refseq = capi.RefSeq(ix, EX_PREFIX)

    def two_iterations(max_events):
        model, used, statuses = capi.Model.default(), [], []
        for _ in range(2):
            acc = capi.ModelAcc()
            res = capi.align_ref_batch(refseq, np.asarray(samples, np.int16), np.array([0, len(samples)], np.uint64), calib1,
                                       [(0, q["smp_st"], q["smp_en"])], stretch, opts=capi.align_opts(max_events=max_events, adaptive=128),
                                       model=model, accumulate=acc)
            statuses.append(int(res["status"][0]))
            used.append(int(acc.read()[0].sum()))
            model, _ = acc.finish(model, 2)
        return model, used, statuses

    model, used, statuses = two_iterations(2000)
    assert ("iteration 1: %d records used" % used[0]) in rows[0] and ("iteration 2: %d records used" % used[1]) in rows[1]
    assert got.pairs().tobytes() == model.pairs().tobytes()
    assert statuses == [capi.ALIGN_TOO_MANY] * 2 and used == [0, 0] and got.pairs().tobytes() == capi.Model.default().pairs().tobytes()
    # without the limit, in this process
    lines = []
    trained = cli.train_model(ix, str(EX_PREFIX), rd, queries, None, 2, 2, False, 0, 0, 2048, 0, lambda *a: lines.append(a), 128)
    model, used, statuses = two_iterations(0)
    assert all(s in (OK, REF_END) for s in statuses) and used[0] > 1000 and [ln[1] for ln in lines] == used
    assert trained.pairs().tobytes() == model.pairs().tobytes() != capi.Model.default().pairs().tobytes()
