"""CPU: banded signal-to-reference DTW below the GPU -- the band checker (tests/dtw_band_check.c) anchored on the reference's committed
results, then k_dtw.hip's banded kernel, the planner and the align pipeline under the lanesim emulator (the existing Makefile.dtw /
Makefile.align builds) against that checker: status, bits of the score, path_len and the whole path.  tests/test_gpu_dtw_band.py
repeats the emulator cases on the gfx950 library and adds the sizes only a GPU can hold."""
import ctypes
import re

import numpy as np
import pytest

import align_cases as ac
import dtw_band_cases as bc
import dtw_cases as dc
from conftest import GOLD, ROOT, locked_make
from dtw_band_check import LEFT_BAND, OK, TOO_NARROW, BandChecker, narrowest, path_halfwidth
from dtw_check import Checker


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD / "dtw_goldens.npz")


@pytest.fixture(scope="module")
def checker():
    return BandChecker()


@pytest.fixture(scope="module")
def full_checker():
    return Checker()


@pytest.fixture(scope="module")
def means(checker):
    return checker.model[:1024]


@pytest.fixture(scope="module")
def sim_dtw_lib():
    from uncalled_amd import capi
    locked_make("-C", str(ROOT / "tests" / "lanesim"), "-f", "Makefile.dtw")
    return capi.load(ROOT / "tests" / "lanesim" / "_build_dtw" / "libuncalled_sim_dtw.so")


@pytest.fixture(scope="module")
def sim_align_lib():
    from uncalled_amd import capi
    locked_make("-C", str(ROOT / "tests" / "lanesim"), "-f", "Makefile.align")
    return capi.load(ROOT / "tests" / "lanesim" / "_build_align" / "libuncalled_sim_align.so")


def gold_case(gold, a):
    ev = gold["events"][int(gold["ev_off"][a]):int(gold["ev_off"][a + 1])]
    km = gold["kmers"][int(gold["km_off"][a]):int(gold["km_off"][a + 1])]
    path = gold["path"][int(gold["path_off"][a]):int(gold["path_off"][a + 1])].astype(np.uint32)
    return ev, km, int(gold["cost"][a]), tuple(map(float, gold["weights"][a])), path


# ------------------------------------------------------------------ 1. the checker, anchored on the reference
def test_checker_reproduces_the_reference_where_the_band_holds_its_path(gold, checker):
    """Every global alignment of the goldens: with the whole matrix in the band, score, mean and path are the reference's; with the
    narrowest band that holds the reference's path (W*), score and path still are; one narrower, the score cannot be smaller."""
    globals_ = [a for a in range(gold["subseq"].size) if int(gold["subseq"][a]) == dc.NONE]
    assert len(globals_) >= 6
    inside = narrower = 0
    for a in globals_:
        ev, km, cost, w, path = gold_case(gold, a)
        rows, cols = km.size, ev.size
        r = checker.dtw(ev, km, cost, *w, max(rows, cols))
        assert r["status"] == OK and r["score_bits"] == int(gold["score_bits"][a]), a
        assert dc.bits(r["mean"]) == int(gold["mean_bits"][a]), a
        assert np.array_equal(r["path"], path) and r["ties"] == int(gold["tie_cells"][a]), a
        w_star = max(path_halfwidth(path, rows, cols), narrowest(rows, cols))
        inside += w_star < rows - 1
        r = checker.dtw(ev, km, cost, *w, w_star)
        assert r["status"] == OK and r["score_bits"] == int(gold["score_bits"][a]) and np.array_equal(r["path"], path), (a, w_star)
        if w_star - 1 >= narrowest(rows, cols):
            r = checker.dtw(ev, km, cost, *w, w_star - 1)
            assert r["status"] == OK and r["score"] >= np.float32(gold["score_bits"][a:a + 1].view(np.float32)[0]), a
            narrower += 1
    assert 3 * inside >= len(globals_) and narrower >= 1, (inside, narrower, len(globals_))


# ------------------------------------------------------------------ 2. the kernel under the emulator
@pytest.mark.lanesim
@pytest.mark.parametrize("cost,weights", [(c, w) for c in (bc.R94P, bc.R94D) for w in bc.WEIGHT_SETS])
def test_kernel_under_the_emulator_equals_the_checker(checker, full_checker, means, sim_dtw_lib, cost, weights):
    seen = {OK: 0, TOO_NARROW: 0}
    for b in bc.shape_batches(means, bc.shapes(), cost, weights):
        _, _, want = bc.check(checker, b, lib=sim_dtw_lib)
        for w in want:
            assert w["status"] in seen, b["name"]       # (finite events never leave the band)
            seen[w["status"]] += 1
        if b["name"].startswith("one below"):
            assert [w["status"] for w in want[1:-1]] == [TOO_NARROW] * (len(want) - 2) and want[0]["status"] == want[-1]["status"] == OK
        if b["band"] == 400:        # W >= R for every shape: unc_dtw_batch on the same input
            from uncalled_amd import capi
            res, paths = bc.run(b, lib=sim_dtw_lib)
            full, fpaths = capi.dtw_batch(b["evs"], b["kms"], capi.DTWParams(dc.NONE, cost, *weights), lib=sim_dtw_lib, full=True)
            assert res.tobytes() == full.tobytes() and all(np.array_equal(p, q) for p, q in zip(paths, fpaths))
            if weights == (0.0, 0.0, 0.0):
                big = max(range(len(want)), key=lambda a: b["evs"][a].size * b["kms"][a].size)
                assert want[big]["ties"] > 0.95 * b["evs"][big].size * b["kms"][big].size
    assert seen[OK] > 300 and seen[TOO_NARROW] > 30, seen


# ------------------------------------------------------------------ 3. a band that binds
@pytest.mark.lanesim
def test_a_band_that_binds_gives_the_banded_optimum(checker, full_checker, means, sim_dtw_lib, sim_align_lib):
    from uncalled_amd import capi
    ev, km = bc.long_stay_case(means)
    W, weights = 4, (1.0, 1.0, 1.0)
    full = full_checker.dtw(ev, km, dc.NONE, dc.R94D, *weights)
    assert path_halfwidth(full["path"], km.size, ev.size) > W           # the premise: the full matrix's path leaves the band
    want = checker.dtw(ev, km, dc.R94D, *weights, W)
    assert want["status"] == OK and want["score"] > full["score"]
    res, paths = capi.dtw_batch([ev], [km], capi.DTWParams(dc.NONE, dc.R94D, *weights), lib=sim_dtw_lib, full=True, band=W)
    bc.assert_equal_to_checker(res, paths, [want])
    assert res["score"][0] > full["score"]
    # the same through align_batch: the events as calibrated samples (range 1, offset 0, digitisation 1 would round them: the raw
    # mode takes int16, so the premise is asserted again on the levels that come back)
    raw = np.round(ev * 8).astype(np.int16)
    calib = capi.make_calib(1, 1.0, 0.0, 8.0)
    o = capi.align_opts(create_events=False, band=W)
    o0 = capi.align_opts(create_events=False)
    r0, lev0, path0 = capi.align_batch(raw, [0, raw.size], calib, [(0, 0, 0)], [km], opts=o0, levels=True, paths=True, lib=sim_align_lib)
    r1, lev1, path1 = capi.align_batch(raw, [0, raw.size], calib, [(0, 0, 0)], [km], opts=o, levels=True, paths=True, lib=sim_align_lib)
    assert np.array_equal(lev0[0], lev1[0])
    assert path_halfwidth(path0[0], km.size, raw.size) > W
    want = checker.dtw(lev1[0], km, dc.R94D, *weights, W)
    assert int(r1["status"][0]) == OK and bc.same_float(r1["dtw"]["score"][0], want["score"]) and np.array_equal(path1[0], want["path"])
    assert r1["dtw"]["score"][0] > r0["dtw"]["score"][0] and path_halfwidth(path1[0], km.size, raw.size) <= W


# ------------------------------------------------------------------ 4. events that are no numbers
@pytest.mark.lanesim
def test_events_that_are_no_numbers_under_the_emulator(checker, means, sim_dtw_lib):
    from uncalled_amd import capi
    b = bc.nonfinite_batch(means)
    want = bc.wanted(checker, b)
    assert want[0]["status"] == LEFT_BAND and 0 < want[0]["path_len"] < 70 + 90 - 1
    res, paths = bc.run(b, lib=sim_dtw_lib)
    bc.assert_equal_to_checker(res, paths, want, b["name"])
    # through the C ABI with sentinels around rooms of the full length: a stopped traceback writes its pairs and nothing else
    evs, kms = b["evs"], b["kms"]
    room = 70 + 90 - 1
    ev, km = np.concatenate(evs), np.concatenate(kms)
    ev_off, km_off = np.arange(4, dtype=np.uint64) * 90, np.arange(4, dtype=np.uint64) * 70
    path_off = (7 + np.arange(4) * (room + 3)).astype(np.uint64)
    path = np.full((int(path_off[-1]) + 32, 2), bc.SENTINEL, np.uint32)
    out = np.zeros(3, capi.DTW_RESULT)
    prm = capi.DTWParams(dc.NONE, b["cost"], *b["weights"])
    rc = sim_dtw_lib.unc_dtw_band_batch(0, 3, ev.ctypes.data, ev_off.ctypes.data, km.ctypes.data, km_off.ctypes.data, ctypes.byref(prm), b["band"], 0,
                                        out.ctypes.data, path.ctypes.data, path_off.ctypes.data, None)
    assert rc == 0
    written = np.zeros(path.shape[0], bool)
    for a, w in enumerate(want):
        at = int(path_off[a])
        assert int(out["status"][a]) == w["status"] and int(out["path_len"][a]) == w["path_len"]
        assert np.array_equal(path[at:at + w["path_len"]], w["path"])
        written[at:at + w["path_len"]] = True
    assert (path[~written] == bc.SENTINEL).all()
    # a room 5 short of a stopped path: LEFT_BAND takes precedence over PATH_TRUNCATED
    n = want[0]["path_len"]
    path_off = np.array([3, 3 + n - 5], np.uint64)
    path = np.full((n + 16, 2), bc.SENTINEL, np.uint32)
    rc = sim_dtw_lib.unc_dtw_band_batch(0, 1, ev.ctypes.data, ev_off.ctypes.data, km.ctypes.data, km_off.ctypes.data, ctypes.byref(prm), b["band"], 0,
                                        out.ctypes.data, path.ctypes.data, path_off.ctypes.data, None)
    assert rc == 0 and int(out["status"][0]) == LEFT_BAND and int(out["path_len"][0]) == n
    assert np.array_equal(path[3:3 + n - 5], want[0]["path"][:n - 5]) and (path[:3] == bc.SENTINEL).all() and (path[3 + n - 5:] == bc.SENTINEL).all()


# ------------------------------------------------------------------ 5. the interface
@pytest.mark.lanesim
def test_interface_under_the_emulator(checker, means, sim_dtw_lib):
    bc.check_argument_errors(sim_dtw_lib)
    bc.check_caller_offsets(sim_dtw_lib, checker, means)
    bc.check_rounds_and_too_large(checker, means, lib=sim_dtw_lib)


def test_header_declares_and_library_exports_the_band_entry_point():
    import __graft_entry__ as g
    from uncalled_amd import capi
    txt = (ROOT / "include" / "uncalled_hip.h").read_text()
    assert "UNC_DTW_BAND_TOO_NARROW 5u" in txt and "UNC_DTW_LEFT_BAND 6u" in txt
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert "unc_dtw_band_batch" in set(re.findall(r"\b(unc_[a-z0-9_]+)\s*\(", code))
    assert re.search(r"uint32_t\s+band;", code)
    L = ctypes.CDLL(str(g.build_hip()))
    assert hasattr(L, "unc_dtw_band_batch")
    assert ctypes.sizeof(capi.AlignOpts) == 32 and capi.AlignOpts.band.offset == 28
    assert ctypes.sizeof(capi.DTWParams) == 20
    assert (capi.DTW_BAND_TOO_NARROW, capi.DTW_LEFT_BAND) == (5, 6)


# ------------------------------------------------------------------ 6. the align pipeline
@pytest.mark.lanesim
def test_align_pipeline_with_a_band_under_the_emulator(checker, sim_align_lib):
    from uncalled_amd import capi
    G = ac.Goldens()
    bc.check_align(G, sim_align_lib, checker)
    # a band with a subsequence mode is refused before anything runs
    c = next(c for c in range(G.n) if int(G.g["subseq"][c]) != dc.NONE)
    o = G.opts(c)
    o.band = 5
    with pytest.raises(capi.UncalledHipError, match="error -1"):
        G.run([c], lib=sim_align_lib, opts=o)


@pytest.mark.lanesim
def test_the_cli_with_a_band_under_the_emulator(checker, sim_align_lib, tmp_path, capsys, monkeypatch):
    """`python -m uncalled_amd dtw ... --band W` in this process with the emulator build in the library's place: the path file equals
    the band checker on the slice's levels; a status of 5 is reported on the line"""
    from conftest import EX_PREFIX
    from uncalled_amd import capi
    from uncalled_amd.__main__ import main
    monkeypatch.setattr(capi, "DEFAULT_LIB", ROOT / "tests" / "lanesim" / "_build_align" / "libuncalled_sim_align.so")
    G = ac.Goldens()
    c = G.idx("example_slice_rev")
    rid = str(np.load(GOLD / "example_read.npz")["read_id"])
    name = capi.Index(EX_PREFIX, lib=sim_align_lib).seq_names()[0]
    qf = tmp_path / "q.txt"
    qf.write_text("%s 10001 14001 %s 6700 7000 -\n" % (rid, name))
    main(["dtw", str(EX_PREFIX), str(GOLD / "example_read.fast5"), str(qf), "-o", str(tmp_path / "p_"), "--band", "64"])
    out = capsys.readouterr().out.strip().split("\n")
    want = checker.dtw(G.seg("levels", "lev_off", c), G.kmers(c), dc.R94D, 1.0, 1.0, 1.0, 64)
    assert want["status"] == OK and len(out) == 1
    assert out[0].split("\t")[:2] == [rid, "%.6g" % float(want["mean"])] and len(out[0].split("\t")) == 3
    rows = [ln.split("\t") for ln in (tmp_path / ("p_%s.txt" % rid)).read_text().strip().split("\n")]
    assert [(int(r[0]), int(r[1])) for r in rows] == [tuple(map(int, p)) for p in want["path"][::-1]]
    qf.write_text("%s 10001 10401 %s 6000 7000 +\n" % (rid, name))          # some 50 events against 996 k-mers
    main(["dtw", str(EX_PREFIX), str(GOLD / "example_read.fast5"), str(qf), "--band", "2"])
    out = capsys.readouterr().out.strip().split("\t")
    assert out[0] == rid and out[-1] == "status 5" and len(out) == 4, out
