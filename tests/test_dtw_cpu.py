"""CPU: the DTW feature below the GPU -- the checker (tests/dtw_check.c) against the committed reference results, the C ABI's
declarations and exports, BwaIndex::get_kmers on the example index, and k_dtw.hip itself under the lanesim emulator (built by
tests/lanesim/Makefile.dtw, a make file of its own: the emulator suite's library does not hold the DTW sources).

The emulator cases past the goldens come from tests/dtw_cases.py, in sizes the emulator can take; tests/test_gpu_dtw.py runs the
full ones (and those only a GPU can hold: indices past 2^16, 4 GiB of back-pointers, two threads).  Measured on the build
container, one process: test_kernel_under_the_emulator_equals_every_golden 8.7 s at the parent commit (7.6 s in the same run as
the following); more alignments than wavefronts 5.5 s, ties at the end cell 2.1 s, ties in every cell and non-finite events 1.3 s,
caller's offsets 0.2 s.  The tests of ties at the end cell, of the caller's offsets and of non-finite events were each seen to
fail under the emulator with the defect they aim at put into k_dtw.hip / unc_dtw.cpp by hand and taken out again (an end cell
chosen by lane or with <=, a base offset ignored, a NaN kept as a lane's candidate).  A row index cut to 16 bits was seen to fail
a 66000 x 1 alignment in a run under the emulator made by hand once: no committed emulator test reaches an index of 2^16 (the GPU
file's do), so nothing here repeats that.  For the test of more alignments than wavefronts no defect was put in: it holds the
queue loop as it is (a wavefront's state left over from its previous alignment would show as a wrong result)."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

import dtw_cases as dc
from conftest import EX_PREFIX, GOLD, ROOT, locked_make
from dtw_check import Checker


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD / "dtw_goldens.npz")


@pytest.fixture(scope="module")
def checker():
    return Checker()


@pytest.fixture(scope="module")
def sim_dtw_lib():
    from uncalled_amd import capi
    locked_make("-C", str(ROOT / "tests" / "lanesim"), "-f", "Makefile.dtw")
    return capi.load(ROOT / "tests" / "lanesim" / "_build_dtw" / "libuncalled_sim_dtw.so")


@pytest.fixture(scope="module")
def means(checker):
    return checker.model[:1024]


def case(gold, a):
    from uncalled_amd import capi
    ev = gold["events"][int(gold["ev_off"][a]):int(gold["ev_off"][a + 1])]
    km = gold["kmers"][int(gold["km_off"][a]):int(gold["km_off"][a + 1])]
    prm = capi.DTWParams(int(gold["subseq"][a]), int(gold["cost"][a]), *map(float, gold["weights"][a]))
    path = gold["path"][int(gold["path_off"][a]):int(gold["path_off"][a + 1])].astype(np.uint32)
    return ev, km, prm, path


def test_goldens_cover_what_they_should(gold):
    n = gold["subseq"].size
    combos = {(int(gold["subseq"][a]), int(gold["cost"][a]), tuple(gold["weights"][a])) for a in range(n)}
    assert len(combos) == 3 * 2 * 3
    shapes = {(int(gold["km_off"][a + 1] - gold["km_off"][a]), int(gold["ev_off"][a + 1] - gold["ev_off"][a])) for a in range(n)}
    assert (1, 1) in shapes and any(r == 1 and c > 1 for r, c in shapes) and any(c == 1 and r > 1 for r, c in shapes)
    assert any(r > 2 * c > 64 for r, c in shapes) and any(c > 2 * r > 64 for r, c in shapes) and (300, 300) in shapes
    assert gold["tie_case"].sum() >= 2 and (gold["tie_cells"][gold["tie_case"] == 1] > 0).all()
    assert {int(st) & 3 for st, _ in gold["kmer_ranges"]} == {0, 1, 2, 3} and {int(en) & 3 for _, en in gold["kmer_ranges"]} == {0, 1, 2, 3}


def test_checker_reproduces_every_golden(gold, checker):
    for a in range(gold["subseq"].size):
        ev, km, prm, path = case(gold, a)
        r = checker.dtw(ev, km, prm.subseq, prm.cost, prm.dw, prm.hw, prm.vw)
        assert r["score_bits"] == int(gold["score_bits"][a]), a
        assert int(r["mean"].view(np.uint32)) == int(gold["mean_bits"][a]), a
        assert r["path_len"] == path.shape[0] and np.array_equal(r["path"], path), a
        assert r["ties"] == int(gold["tie_cells"][a]), a


def test_model_tables_and_costs_equal_the_reference(gold, checker):
    from uncalled_amd import capi
    means, v2, ln = capi.dtw_model_tables()
    assert np.array_equal(means.view(np.uint32), gold["model_mean_bits"])
    # the template model is the mapper's complement model with the rows complemented (k ^ 0x3FF)
    for k, e, p, d in zip(gold["cost_kmer"], gold["cost_event"], gold["cost_r94p_bits"], gold["cost_r94d_bits"]):
        assert int(checker.cost(0, k, e).view(np.uint32)) == int(p), (k, e)
        assert int(checker.cost(1, k, e).view(np.uint32)) == int(d), (k, e)
    # `abs` in the reference's cost is the float overload: the first point lies 0.37 off its k-mer's mean
    assert 0.3 < float(gold["cost_r94d_bits"][:1].view(np.float32)[0]) < 0.45


def test_header_declares_and_library_exports_the_dtw_entry_points():
    import __graft_entry__ as g
    txt = (ROOT / "include" / "uncalled_hip.h").read_text()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    syms = set(re.findall(r"\b(unc_[a-z0-9_]+)\s*\(", txt))
    assert {"unc_dtw_batch", "unc_ref_kmers", "unc_dtw_last_timing", "unc_dtw_model_tables"} <= syms
    for name in ("UNC_DTW_EVENT_GLOB", "UNC_DTW_EVENT_QSUB", "UNC_DTW_EVENT_RSUB", "UNC_DTW_RAW_GLOB", "UNC_DTW_RAW_QSUB", "UNC_DTW_RAW_RSUB",
                 "UNC_DTW_TOO_LARGE", "unc_dtw_params_t", "unc_dtw_result_t"):
        assert name in txt, name
    assert "k_dtw.hip" in g.HIP_SOURCES
    L = ctypes.CDLL(str(g.build_hip()))      # hipcc cross-compiles for gfx950 without a GPU
    for s in ("unc_dtw_batch", "unc_ref_kmers", "unc_dtw_last_timing", "unc_dtw_model_tables"):
        assert hasattr(L, s), s


def test_ref_kmers_equals_the_reference(gold, sim_dtw_lib):
    """capi.ref_kmers is host code behind the index handle: here through the emulator build of the library (no GPU to load an
    index onto); tests/test_gpu_dtw.py repeats it through the gfx950 library."""
    from uncalled_amd import capi
    ix = capi.Index(EX_PREFIX, lib=sim_dtw_lib)
    off = gold["kmers_off"]
    for r, (st, en) in enumerate(gold["kmer_ranges"]):
        want_f, want_r = gold["kmers_fwd"][int(off[r]):int(off[r + 1])], gold["kmers_rev"][int(off[r]):int(off[r + 1])]
        assert np.array_equal(capi.ref_kmers(ix, EX_PREFIX, 0, int(st), int(en), True), want_f), (st, en)
        assert np.array_equal(capi.ref_kmers(ix, EX_PREFIX, 0, int(st), int(en), False), want_r), (st, en)
    with pytest.raises(capi.UncalledHipError):
        capi.ref_kmers(ix, EX_PREFIX, 0, 9000, 10001)
    with pytest.raises(capi.UncalledHipError):
        capi.ref_kmers(ix, EX_PREFIX, 1, 0, 100)


@pytest.mark.lanesim
def test_kernel_under_the_emulator_equals_every_golden(gold, sim_dtw_lib):
    """k_dtw.hip on the CPU emulator: the goldens of one parameter set per batch (mixed shapes share a launch), all at once, in
    rounds forced by a small workspace, and with a workspace below the largest alignment."""
    from uncalled_amd import capi
    n = gold["subseq"].size
    groups, seen = {}, dict(rounds=0, too_large=0)
    for a in range(n):
        groups.setdefault((int(gold["subseq"][a]), int(gold["cost"][a]), tuple(map(float, gold["weights"][a]))), []).append(a)
    for (subseq, cost, w), members in groups.items():
        prm = capi.DTWParams(subseq, cost, *w)
        evs, kms, paths = zip(*[(c[0], c[1], c[3]) for c in (case(gold, a) for a in members)])
        for ws in (0, 20000):
            res, got = capi.dtw_batch(evs, kms, prm, workspace_bytes=ws, lib=sim_dtw_lib, full=True)
            _, rounds, held = capi.dtw_last_timing(sim_dtw_lib)
            if ws:
                assert held <= ws
                seen["rounds"] = max(seen["rounds"], rounds)
            for a, r, p, want in zip(members, res, got, paths):
                words = 64 * ((kms[members.index(a)].size + 63) // 64) * ((evs[members.index(a)].size + 63 + 15) // 16)
                if ws and words * 4 > ws:
                    assert r["status"] == capi.DTW_TOO_LARGE and p is None, a
                    seen["too_large"] += 1
                    continue
                assert r["status"] == capi.DTW_OK, a
                assert int(r["score"].view(np.uint32)) == int(gold["score_bits"][a]), a
                assert int(r["mean_score"].view(np.uint32)) == int(gold["mean_bits"][a]), a
                assert int(r["path_len"]) == want.shape[0] and np.array_equal(p, want), a
        scores, _, none = capi.dtw_batch(evs, kms, prm, paths=False, lib=sim_dtw_lib)
        assert none is None and np.array_equal(scores.view(np.uint32), gold["score_bits"][members])
    assert seen["rounds"] >= 3 and seen["too_large"] >= 1, seen


@pytest.mark.lanesim
def test_argument_errors_under_the_emulator(sim_dtw_lib):
    from uncalled_amd import capi
    ev, km = np.full(4, 90, np.float32), np.arange(4, dtype=np.uint16)
    for evs, kms, prm in (([ev[:0]], [km], capi.DTW_EVENT_GLOB), ([ev], [km[:0]], capi.DTW_EVENT_GLOB),
                          ([ev], [km + 1021], capi.DTW_EVENT_GLOB), ([ev], [km], capi.DTWParams(3, 0, 1, 1, 1)),
                          ([ev], [km], capi.DTWParams(0, 2, 1, 1, 1))):
        with pytest.raises(capi.UncalledHipError, match="error -1"):
            capi.dtw_batch(evs, kms, prm, lib=sim_dtw_lib)


def test_checker_counts_the_minimal_cells_of_the_line_it_scans(checker, means):
    """one event on the mean of k-mer `a`, r94d: the last column (ROW) is |mean(k) - mean(a)| row by row"""
    a, b, c = (int(k) for k in np.argsort(means)[[100, 500, 900]])
    ev = means[[a]]
    for km, n_min, last in (([a, b, a, c, a], 3, True), ([a, b, a, c], 2, False), ([b, c, b], 2, True), ([c], 1, True)):
        r = checker.dtw(ev, np.array(km, np.uint16), dc.ROW, dc.R94D, 1, 1, 1)
        assert (r["end_min_cells"], r["last_is_min"]) == (n_min, last), km
        assert tuple(r["path"][0]) == (0, len(km) - 1 if last else km.index(a)), km
        r = checker.dtw(means[km], np.array([a], np.uint16), dc.COL, dc.R94D, 1, 1, 1)      # the mirror image
        assert (r["end_min_cells"], r["last_is_min"]) == (n_min, last), km
        assert tuple(r["path"][0]) == (len(km) - 1 if last else km.index(a), 0), km
        r = checker.dtw(ev, np.array(km, np.uint16), dc.NONE, dc.R94D, 1, 1, 1)
        assert (r["end_min_cells"], r["last_is_min"]) == (0, False)
    nan = np.array([np.nan], np.float32)        # a line of NaN has no minimum
    r = checker.dtw(nan, np.array([a, b], np.uint16), dc.ROW, dc.R94D, 1, 1, 1)
    assert (r["end_min_cells"], r["last_is_min"]) == (0, False) and tuple(r["path"][0]) == (0, 1)


@pytest.mark.lanesim
def test_more_alignments_than_wavefronts_under_the_emulator(checker, means, sim_dtw_lib):
    """200 alignments of at most 40 x 40 on the emulator's grid of 16 x 4 wavefronts, in every subseq x cost: a wavefront goes
    round the queue loop of k_dtw more than once"""
    from uncalled_amd import capi
    for b in dc.queue_batches(means, 200, 50, 40):
        assert len(b["evs"]) > 16 * 4
        dc.check(checker, b, lib=sim_dtw_lib)
        assert capi.dtw_last_timing(sim_dtw_lib)[1] == 1


@pytest.mark.lanesim
def test_offsets_as_a_caller_may_give_them_under_the_emulator(checker, means, sim_dtw_lib):
    dc.check_caller_offsets(sim_dtw_lib, checker, means)
    dc.check_no_paths_with_a_too_large_member(checker, means, lib=sim_dtw_lib)


@pytest.mark.lanesim
def test_ties_at_the_end_cell_under_the_emulator(checker, means, sim_dtw_lib):
    for b in dc.end_tie_batches(means):
        res, paths, want = dc.check(checker, b, lib=sim_dtw_lib)
        dc.assert_end_ties(b, want)
        assert [tuple(int(x) for x in p[0]) for p in paths] == b["end"], b["name"]


@pytest.mark.lanesim
def test_ties_in_every_cell_and_events_that_are_no_numbers_under_the_emulator(checker, means, sim_dtw_lib):
    rows, cols = 150, 130
    for b in dc.zero_weight_batches(means, rows, cols):
        _, _, want = dc.check(checker, b, lib=sim_dtw_lib)
        # (99 % at the GPU file's 1000 x 900; at 150 x 130 the first row and column, next to the border's MAX_COST, are 1.4 % of the cells)
        assert want[0]["ties"] > 0.95 * rows * cols, b["name"]
    for b in dc.rounded_batches(means, rows, cols, 1.0):
        _, _, want = dc.check(checker, b, lib=sim_dtw_lib)
        assert want[0]["ties"] >= 0.01 * rows * cols, b["name"]
    for b in dc.nonfinite_batches(means, rows, cols):
        dc.check(checker, b, lib=sim_dtw_lib)
    b = dc.nan_before_the_end_batch(means)
    _, paths, want = dc.check(checker, b, lib=sim_dtw_lib)
    assert want[0]["score"] == 0.0 and want[0]["end_min_cells"] == 1 and not want[0]["last_is_min"]
    assert tuple(int(x) for x in paths[0][0]) == b["end"][0]
