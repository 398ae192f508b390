"""GPU: banded signal-to-reference DTW on the gfx950 library against the band checker (tests/dtw_band_check.c, anchored on the
reference's results by tests/test_dtw_band_cpu.py): the emulator file's cases, then what only a GPU holds -- more alignments than
the launch has wavefronts, indices past 2^16, a 20000 x 30000 alignment with linear memory, two threads, the command line."""
import ctypes
import subprocess
import sys

import numpy as np
import pytest

import align_cases as ac
import dtw_band_cases as bc
import dtw_cases as dc
from conftest import EX_PREFIX, GOLD, ROOT
from dtw_band_check import LEFT_BAND, OK, TOO_NARROW, BandChecker, narrowest, path_halfwidth
from dtw_check import Checker

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def checker():
    return BandChecker()


@pytest.fixture(scope="module")
def means(checker):
    return checker.model[:1024]


# ------------------------------------------------------------------ 1. the emulator file's cases
@pytest.mark.parametrize("cost,weights", [(c, w) for c in (bc.R94P, bc.R94D) for w in bc.WEIGHT_SETS])
def test_shapes_and_bands_equal_the_checker(hip_lib, checker, means, cost, weights):
    from uncalled_amd import capi
    seen = {OK: 0, TOO_NARROW: 0}
    for b in bc.shape_batches(means, bc.shapes(), cost, weights):
        _, _, want = bc.check(checker, b)
        for w in want:
            assert w["status"] in seen, b["name"]
            seen[w["status"]] += 1
        if b["band"] == 400:        # W >= R for every shape: unc_dtw_batch on the same input
            res, paths = bc.run(b)
            full, fpaths = capi.dtw_batch(b["evs"], b["kms"], capi.DTWParams(dc.NONE, cost, *weights), full=True)
            assert res.tobytes() == full.tobytes() and all(np.array_equal(p, q) for p, q in zip(paths, fpaths))
    assert seen[OK] > 300 and seen[TOO_NARROW] > 30, seen


def test_a_band_that_binds_gives_the_banded_optimum(hip_lib, checker, means):
    from uncalled_amd import capi
    ev, km = bc.long_stay_case(means)
    W, weights = 4, (1.0, 1.0, 1.0)
    full = Checker().dtw(ev, km, dc.NONE, dc.R94D, *weights)
    assert path_halfwidth(full["path"], km.size, ev.size) > W
    want = checker.dtw(ev, km, dc.R94D, *weights, W)
    assert want["status"] == OK and want["score"] > full["score"]
    res, paths = capi.dtw_batch([ev], [km], capi.DTWParams(dc.NONE, dc.R94D, *weights), full=True, band=W)
    bc.assert_equal_to_checker(res, paths, [want])
    raw = np.round(ev * 8).astype(np.int16)
    calib = capi.make_calib(1, 1.0, 0.0, 8.0)
    r0, lev0, path0 = capi.align_batch(raw, [0, raw.size], calib, [(0, 0, 0)], [km], opts=capi.align_opts(create_events=False), levels=True,
                                       paths=True)
    r1, lev1, path1 = capi.align_batch(raw, [0, raw.size], calib, [(0, 0, 0)], [km], opts=capi.align_opts(create_events=False, band=W),
                                       levels=True, paths=True)
    assert path_halfwidth(path0[0], km.size, raw.size) > W
    want = checker.dtw(lev1[0], km, dc.R94D, *weights, W)
    assert int(r1["status"][0]) == OK and bc.same_float(r1["dtw"]["score"][0], want["score"]) and np.array_equal(path1[0], want["path"])
    assert r1["dtw"]["score"][0] > r0["dtw"]["score"][0]


def test_events_that_are_no_numbers(hip_lib, checker, means):
    b = bc.nonfinite_batch(means)
    want = bc.wanted(checker, b)
    assert want[0]["status"] == LEFT_BAND
    res, paths = bc.run(b)
    bc.assert_equal_to_checker(res, paths, want, b["name"])
    for cost, weights in ((bc.R94P, (2.0, 1.0, 100.0)), (bc.R94P, (0.0, 0.0, 0.0))):
        bc.check(checker, bc.nonfinite_batch(means, rows=700, cols=900, band=40, cost=cost, weights=weights))


def test_interface(hip_lib, checker, means):
    bc.check_argument_errors(hip_lib)
    bc.check_caller_offsets(hip_lib, checker, means)
    bc.check_rounds_and_too_large(checker, means)


def test_align_pipeline_with_a_band(hip_lib, checker):
    bc.check_align(ac.Goldens(), None, checker)


def test_the_host_module_takes_a_trailing_band(hip_lib, checker, means):
    from uncalled_amd import _uncalled_amd as unc
    ev, km = bc.long_stay_case(means)
    prm = unc.DTWParams(0, 1.0, 1.0, 1.0)
    want = checker.dtw(ev, km, bc.R94D, 1.0, 1.0, 1.0, 4)
    d = unc.DTWr94d(ev.tolist(), km.tolist(), prm, 4)
    assert bc.same_float(d.score(), want["score"]) and [tuple(p) for p in d.get_path()] == [tuple(map(int, p)) for p in want["path"]]
    full = unc.DTWr94d(ev.tolist(), km.tolist(), prm)
    assert full.score() < d.score() and unc.DTWr94d(ev.tolist(), km.tolist(), prm, band=0).score() == full.score()
    with pytest.raises(RuntimeError, match="too narrow"):
        unc.DTWr94p(ev[:3].tolist(), km.tolist(), prm, 2)


# ------------------------------------------------------------------ 2. more alignments than wavefronts
def test_more_alignments_than_wavefronts(hip_lib, checker, means):
    """three times more alignments than the launch has wavefronts (16 per compute unit), cycling 50 small cases: a wavefront goes
    round the queue loop again with the banded state of its previous alignment left over"""
    import torch
    from uncalled_amd import capi
    n = 3 * 16 * torch.cuda.get_device_properties(0).multi_processor_count + 7
    q = dc.queue_batches(means, n, 50, 40)[0]
    assert q["subseq"] == dc.NONE
    distinct = {}
    for a, d in enumerate(q["of"]):
        distinct.setdefault(d, a)
    for W in (3, 40):
        done = {d: checker.dtw(q["evs"][a], q["kms"][a], bc.R94D, 2.0, 1.0, 100.0, W) for d, a in distinct.items()}
        b = bc.batch(f"queue W {W}", q["evs"], q["kms"], bc.R94D, (2.0, 1.0, 100.0), W)
        res, paths = bc.run(b)
        assert capi.dtw_last_timing()[1] == 1
        bc.assert_equal_to_checker(res, paths, [done[d] for d in q["of"]], b["name"])
        assert {w["status"] for w in done.values()} == ({OK, TOO_NARROW} if W == 3 else {OK})


# ------------------------------------------------------------------ 3. indices past 2^16
@pytest.mark.parametrize("rows,cols,band", [(70000, 70000, 5), (66000, 200, 329), (200, 66000, 3)])
def test_row_and_column_indices_past_65536(hip_lib, checker, means, rows, cols, band):
    rng = np.random.default_rng(31)
    assert band >= narrowest(rows, cols) and (rows != 66000 or band == narrowest(rows, cols))
    km = rng.integers(0, 1024, rows).astype(np.uint16)
    ev = (means[km[(np.arange(cols, dtype=np.int64) * rows) // cols]] + 0.5 * rng.standard_normal(cols)).astype(np.float32)
    b = bc.batch(f"long {rows} x {cols}", [ev], [km], bc.R94D, (2.0, 1.0, 100.0), band)
    _, paths, want = bc.check(checker, b)
    assert want[0]["status"] == OK and want[0]["path_len"] >= max(rows, cols) and tuple(paths[0][-1]) == (0, 0)


# ------------------------------------------------------------------ 4. a whole read: 20000 k-mers x 30000 events
def test_a_whole_read_in_linear_memory(hip_lib, checker, means):
    from uncalled_amd import capi
    rows, cols, W = 20000, 30000, 128
    rng = np.random.default_rng(32)
    km = rng.integers(0, 1024, rows).astype(np.uint16)
    ev = dc.follow(rng, means, km, cols)
    b = bc.batch("whole read", [ev], [km], bc.R94P, (2.0, 1.0, 100.0), W)
    _, paths, want = bc.check(checker, b)
    ms, rounds, held = capi.dtw_last_timing()
    print(f"20000 x 30000 at W = 128: kernel {ms:.2f} ms, {held} bytes of back-pointers, path of {want[0]['path_len']}")
    assert want[0]["status"] == OK and rounds == 1
    assert held == bc.band_crumb_bytes(rows, cols, W)
    assert held <= cols * (2 * W + 1) + 64 * (rows + cols) + 4096
    assert held < dc.crumb_bytes(rows, cols) / 10 and dc.crumb_bytes(rows, cols) > 140e6


# ------------------------------------------------------------------ 5. two threads
def test_two_threads_each_on_a_stream_of_its_own(hip_lib, checker, means):
    """unc_dtw_band_batch from two threads at once: one held to a workspace of four alignments (3 rounds or more), one free (1 round);
    each gets the checker's results and unc_dtw_last_timing tells each of its own call"""
    import threading

    import torch
    from uncalled_amd import capi
    b = bc.rounds_batch(means)
    want = bc.wanted(checker, b)
    bc.run(b)       # (the model's upload, not raced here)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    barrier = threading.Barrier(2, timeout=60)
    out = [None, None]

    def work(t, ws):
        try:
            barrier.wait()
            res, paths = bc.run(b, workspace_bytes=ws, stream=streams[t].cuda_stream)
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
        bc.assert_equal_to_checker(out[t][0], out[t][1], want, f"thread {t}")
    assert out[0][2][1] >= 3 and out[0][2][2] <= b["workspace"] and out[1][2][1] == 1 and out[1][2][2] == sum(b["sizes"])


# ------------------------------------------------------------------ 6. the command line
def test_the_cli_with_a_band_in_a_fresh_process(hip_lib, checker, tmp_path):
    """`python -m uncalled_amd dtw ... --band 64` in a child process: path file and mean score equal capi.align_batch with the same band
    (and the band checker on its levels); without --band the line and the path file are the full matrix's, three fields as before"""
    from uncalled_amd import capi
    G = ac.Goldens()
    ex = np.load(GOLD / "example_read.npz")
    rid = str(ex["read_id"])
    ix = capi.Index(EX_PREFIX)
    qf = tmp_path / "q.txt"
    qf.write_text("%s 10001 14001 %s 6700 7000 +\n" % (rid, ix.seq_names()[0]))
    km = capi.ref_kmers(ix, EX_PREFIX, 0, 6700, 7000, fwd=True)
    for band in (64, 0):
        prefix = str(tmp_path / ("out%d_" % band))
        cmd = [sys.executable, "-m", "uncalled_amd", "dtw", str(EX_PREFIX), str(GOLD / "example_read.fast5"), str(qf), "-o", prefix]
        run = subprocess.run(cmd + (["--band", str(band)] if band else []), cwd=str(ROOT), capture_output=True, text=True, timeout=300)
        assert run.returncode == 0, run.stderr[-2000:]
        res, levs, paths = capi.align_batch(G.raw, G.offsets, G.calib, [(3, 10001, 14001)], [km], levels=True, paths=True,
                                            opts=capi.align_opts(max_events=50000, band=band))
        assert int(res["status"][0]) == OK
        fields = run.stdout.strip().split("\n")
        assert len(fields) == 1 and fields[0].split("\t")[:2] == [rid, "%.6g" % float(res[0]["dtw"]["mean_score"])]
        assert len(fields[0].split("\t")) == 3          # (a status is reported only when it is 5 or 6)
        rows = [ln.split("\t") for ln in open(prefix + rid + ".txt").read().strip().split("\n")]
        assert [(int(r[0]), int(r[1])) for r in rows] == [tuple(map(int, p)) for p in paths[0][::-1]]
        if band:
            w = checker.dtw(levs[0], km, bc.R94D, 1.0, 1.0, 1.0, band)
            assert np.array_equal(paths[0], w["path"]) and bc.same_float(res[0]["dtw"]["score"], w["score"])
        else:           # without --band: the full matrix, as the committed golden of this slice has it
            rev = capi.ref_kmers(ix, EX_PREFIX, 0, 6700, 7000, fwd=False)
            full = capi.align_batch(G.raw, G.offsets, G.calib, [(3, 10001, 14001)], [rev], levels=True, paths=True)
            G.check(G.idx("example_slice_rev"), full[0][0], full[1][0], full[2][0])


def test_the_cli_reports_a_band_too_narrow(hip_lib, tmp_path, capsys):
    from uncalled_amd import capi
    from uncalled_amd.__main__ import main
    rid = str(np.load(GOLD / "example_read.npz")["read_id"])
    qf = tmp_path / "q.txt"
    qf.write_text("%s 10001 10401 %s 6000 7000 +\n" % (rid, capi.Index(EX_PREFIX).seq_names()[0]))        # some 50 events, 996 k-mers
    main(["dtw", str(EX_PREFIX), str(GOLD / "example_read.fast5"), str(qf), "--band", "2"])
    out = capsys.readouterr().out.strip().split("\t")
    assert out[0] == rid and out[-1] == "status 5" and len(out) == 4, out
