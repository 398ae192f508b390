"""CPU: the adaptive-band DTW with an open end below the GPU -- the checker (tests/dtw_adapt_check.c) anchored on tests/dtw_check.c
and the reference's committed results, then k_dtw_adapt.hip, the planner and the align pipeline under the lanesim emulator (the
existing Makefile.dtw / Makefile.align builds) against that checker: status, bits of the score, path_len and the whole path.
Section 2b takes the kernel to its width edges at B = 64, 128 and 256 (dtw_adapt_cases.py: rows around B / 2, B and above; sweeps
that end early, at every residue of the two partial flushes; non-finite events at column 0 and column cols - 1; paths of 63, 64, 65
and 128 pairs with two and four cells a lane) and states two properties of the sweep by the checker alone; section 4 takes the
adaptive band through a custom model, the training accumulator, the pile-up, two rounds, the other align options and a path without
a start (adapt_pipeline_cases.py).  tests/test_gpu_dtw_adapt.py repeats the emulator cases on the gfx950 library and adds the sizes only a GPU can hold.  Nothing here
opens a GPU."""
import subprocess

import numpy as np
import pytest

import adapt_pipeline_cases as apc
import align_cases as ac
import dtw_adapt_cases as xc
import dtw_cases as dc
from conftest import EX_PREFIX, GOLD, ROOT, build_lock
from dtw_adapt_check import LEFT_BAND, OK, REF_END, AdaptChecker
from dtw_check import Checker

SIM_DIR = ROOT / "tests" / "lanesim"


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD / "dtw_goldens.npz")


@pytest.fixture(scope="module")
def checker():
    return AdaptChecker()


@pytest.fixture(scope="module")
def means(checker):
    return checker.model[:1024]


def sim(makefile, lib):
    """the emulator library of `makefile`, rebuilt if a source it includes is newer (the Makefiles name the compiled sources only)"""
    import __graft_entry__ as g
    from uncalled_amd import capi
    so = SIM_DIR / lib
    with build_lock():
        sources = [g.CSRC / f for f in g.HIP_INCLUDED + g.HIP_SOURCES] + list(g.CSRC.glob("*.h"))
        stale = so.exists() and any(f.stat().st_mtime > so.stat().st_mtime for f in sources)
        subprocess.run(["make", "-s", "-C", str(SIM_DIR), "-f", makefile] + (["-B"] if stale else []), check=True)
    L = capi.load(so)
    assert hasattr(L, "unc_dtw_adapt_batch")
    return L


@pytest.fixture(scope="module")
def sim_dtw_lib():
    return sim("Makefile.dtw", "_build_dtw/libuncalled_sim_dtw.so")


@pytest.fixture(scope="module")
def sim_align_lib():
    return sim("Makefile.align", "_build_align/libuncalled_sim_align.so")


# ------------------------------------------------------------------ 1. the checker, anchored on what the project trusts
def test_full_matrix_open_end_equals_dtw_check_where_the_end_is_the_last_cell(gold, checker):
    """Every global alignment of the goldens whose open end is the last cell: score bits and path equal tests/dtw_check.c with
    UNC_DTW_NONE, which the reference's committed results anchor."""
    full_checker = Checker()
    globals_ = [a for a in range(gold["subseq"].size) if int(gold["subseq"][a]) == dc.NONE]
    held = 0
    for a in globals_:
        ev = gold["events"][int(gold["ev_off"][a]):int(gold["ev_off"][a + 1])]
        km = gold["kmers"][int(gold["km_off"][a]):int(gold["km_off"][a + 1])]
        cost, w = int(gold["cost"][a]), tuple(map(float, gold["weights"][a]))
        f = checker.full(ev, km, cost, *w)
        if f["end_row"] != km.size - 1:
            continue
        held += 1
        want = full_checker.dtw(ev, km, dc.NONE, cost, *w)
        assert f["status"] == REF_END and f["score_bits"] == want["score_bits"] == int(gold["score_bits"][a]), a
        assert np.array_equal(f["path"], want["path"]), a
    assert held >= 2, (held, len(globals_))


def random_shapes(means, seed=51):
    rng = np.random.default_rng(seed)
    shapes = [(1, 1), (1, 40), (40, 1), (5, 5), (70, 70), (200, 300), (300, 90), (33, 257)]
    shapes += [(int(rng.integers(1, 260)), int(rng.integers(1, 260))) for _ in range(12)]
    for n, (r, c) in enumerate(shapes):
        km = rng.integers(0, 1024, r).astype(np.uint16)
        ev = dc.follow(rng, means, km[:max(1, 2 * r // 3)], c) if n % 3 else rng.uniform(60, 130, c).astype(np.float32)
        yield ev, km


@pytest.mark.parametrize("cost,weights", [(c, w) for c in (xc.R94P, xc.R94D) for w in xc.WEIGHT_SETS])
def test_an_adaptive_cell_is_never_below_its_full_matrix_value(checker, means, cost, weights):
    """finite events: the monotonicity the header states, over every computed cell of random shapes at every width"""
    cells = 0
    for ev, km in random_shapes(means):
        f = checker.full(ev, km, cost, *weights, cells=True)["cells"]
        for B in (64, 128, 256):
            a = checker.dtw(ev, km, cost, *weights, B, cells=True)
            for (i, j), v in a["cells"].items():
                assert v >= f[i, j], (km.size, ev.size, B, i, j, v, f[i, j])
            cells += len(a["cells"])
            if a["end_row"] is not None:
                assert a["score"] >= checker.full(ev, km, cost, *weights)["score"] or a["status"] == LEFT_BAND
    assert cells > 100000


FOLLOW_FAMILY = [(60 + 17 * s, int((60 + 17 * s) * 1.5) + s, 100 + s) for s in range(20)]        # k-mers followed, events, seed


@pytest.mark.parametrize("cost,weights", [(c, w) for c in (xc.R94P, xc.R94D) for w in xc.WEIGHT_SETS])
def test_on_events_that_follow_their_kmers_the_adaptive_path_is_the_full_matrix_open_end_path(checker, means, cost, weights):
    """B = 256.  The family: for s = 0 .. 19, seed 100 + s, U = 60 + 17 s k-mers followed by floor(1.5 U) + s events made with
    dtw_cases.follow (noise 1.5; stays and skips as its sorted random indices give them), the stretch 1.5 times too long
    (floor(1.5 U) k-mers).  For every case, both costs and both weight sets, the adaptive path equals the full-matrix open-end path in
    every pair and the score in every bit: a condition on the inputs, verified here by the checker alone."""
    for used, cols, seed in FOLLOW_FAMILY:
        rng = np.random.default_rng(seed)
        km = rng.integers(0, 1024, int(used * 1.5)).astype(np.uint16)
        ev = dc.follow(rng, means, km[:used], cols)
        a, f = checker.dtw(ev, km, cost, *weights, 256), checker.full(ev, km, cost, *weights)
        assert a["status"] == f["status"] == OK, (seed, a["status"], f["status"])
        assert a["score_bits"] == f["score_bits"] and np.array_equal(a["path"], f["path"]), (seed, a["end_row"], f["end_row"])


# ------------------------------------------------------------------ 2. the kernel under the emulator
@pytest.mark.lanesim
@pytest.mark.parametrize("cost,weights", [(c, w) for c in (xc.R94P, xc.R94D) for w in xc.WEIGHT_SETS])
def test_kernel_under_the_emulator_equals_the_checker(checker, means, sim_dtw_lib, cost, weights):
    seen = set()
    for b in xc.shape_batches(means, cost, weights):
        _, paths, want = xc.check(checker, b, lib=sim_dtw_lib)
        seen |= {w["status"] for w in want}
        if b["name"].startswith("shapes"):
            lens = [w["path_len"] for w in want]
            assert lens[-3:] == [63, 64, 65] and want[5]["lo"].max() > 0, lens
        if b["name"].startswith("k-mers run out") and weights == (1.0, 1.0, 1.0):      # (with dw = 2 hw an early end is cheaper)
            assert want[0]["status"] == REF_END and want[2]["status"] == OK and want[2]["end_row"] < 200
    assert seen == {OK, REF_END}
    ev, km = xc.case_of_path_len(checker, means, 128, cost, weights)
    _, _, want = xc.check(checker, xc.batch("a path of 128 pairs", [ev], [km], cost, weights, 64), lib=sim_dtw_lib)
    assert want[0]["path_len"] == 128


@pytest.mark.lanesim
def test_a_band_that_binds_under_the_emulator(checker, means, sim_dtw_lib):
    xc.check_binding(checker, means, lib=sim_dtw_lib)


@pytest.mark.lanesim
def test_events_that_are_no_numbers_and_ties_under_the_emulator(checker, means, sim_dtw_lib):
    b = xc.nonfinite_batch(means)
    _, _, want = xc.check(checker, b, lib=sim_dtw_lib)
    assert want[0]["status"] == LEFT_BAND       # behind a NaN column no score compares: the band moves by parity alone
    for cost, weights in ((xc.R94P, (2.0, 1.0, 100.0)), (xc.R94P, (0.0, 0.0, 0.0)), (xc.R94D, (0.0, 0.0, 0.0))):
        xc.check(checker, xc.nonfinite_batch(means, cost=cost, weights=weights), lib=sim_dtw_lib)
    b = xc.all_equal_batch(means)
    _, _, want = xc.check(checker, b, lib=sim_dtw_lib)
    lo = want[0]["lo"]
    free = lo[:-1] + 64 - 1 < 150 - 1           # (once the band holds the last row it stays)
    assert free.sum() > 100 and np.array_equal(np.diff(lo), np.where(free, np.arange(lo.size - 1) % 2, 0))     # ties: right after even d, down after odd d
    xc.check(checker, xc.batch("all ties", b["evs"], b["kms"], xc.R94P, (0.0, 0.0, 0.0), 128), lib=sim_dtw_lib)


@pytest.mark.lanesim
def test_interface_under_the_emulator(checker, means, sim_dtw_lib, sim_align_lib):
    xc.check_argument_errors(sim_align_lib)
    xc.check_caller_offsets(sim_dtw_lib, checker, means)
    xc.check_rounds_and_too_large(checker, means, lib=sim_dtw_lib)


# ------------------------------------------------------------------ 2b. the band's width edges, two and four cells a lane
def test_the_sweep_always_computes_a_cell_of_the_last_column(checker, means):
    """The checker alone.  The last column's row d - (cols - 1) goes down one row an anti-diagonal and the band at most one, until it
    holds the last row and stays: the row catches up before the sweep ends.  So for valid inputs "no cell of column C - 1 was
    computed" (UNC_DTW_LEFT_BAND with score 0 and path_len 0) does not occur: every shape up to 40 x 40 at B = 64, and taller ones."""
    none, n = xc.sweep_without_last_column(checker, means)
    assert none == 0 and n >= 2 * 40 * 40


def test_an_early_end_comes_after_an_odd_number_of_anti_diagonals(checker, means):
    """The checker alone.  The sweep ends early at the first d whose last-column row lies below the band.  Then d - 1 had that row as
    its only present cell (i_t == i_b), the move after it was a tie that went right, and ties go right after even d - 1: d, the
    number of anti-diagonals computed, is odd.  So of n_done modulo 64, the residues 0 and 16 come only from sweeps that run to
    their end (dtw_adapt_cases.full_sweep_case), and case_of_n_done finds nothing for them."""
    seen = set()
    for B in (64, 128, 256):
        for ev, km in list(xc.early_end_family(means, B))[::7]:
            for cost, weights in ((xc.R94D, (1.0, 1.0, 1.0)), (xc.R94P, (2.0, 1.0, 100.0))):
                w = xc.n_done_case(checker, ev, km, B, cost, weights)
                if w is not None:
                    assert w["lo"].size % 2 == 1, (B, km.size, ev.size, w["lo"].size)
                    seen.add(w["lo"].size % 64)
    assert len(seen) >= 16
    with pytest.raises(AssertionError, match="no case whose sweep ends early"):
        xc.case_of_n_done(checker, means, 64, 16, xc.R94D, (1.0, 1.0, 1.0))


@pytest.mark.lanesim
@pytest.mark.parametrize("B", [64, 128, 256])
def test_band_edges_under_the_emulator(checker, means, sim_dtw_lib, B):
    xc.check_edges(checker, means, B, lib=sim_dtw_lib)


@pytest.mark.lanesim
@pytest.mark.parametrize("B", [64, 128, 256])
def test_early_end_of_the_sweep_under_the_emulator(checker, means, sim_dtw_lib, B):
    xc.check_early_end(checker, means, B, lib=sim_dtw_lib)


@pytest.mark.lanesim
def test_non_finite_events_at_the_first_and_last_column_under_the_emulator(checker, means, sim_dtw_lib):
    xc.check_nonfinite_ends(checker, means, lib=sim_dtw_lib)


@pytest.mark.lanesim
@pytest.mark.parametrize("B", [128, 256])
def test_path_length_residues_with_several_cells_a_lane_under_the_emulator(checker, means, sim_dtw_lib, B):
    xc.check_path_residues(checker, means, B, lib=sim_dtw_lib)


# ------------------------------------------------------------------ 3. the align pipeline
@pytest.mark.lanesim
def test_align_pipeline_on_the_example_read_under_the_emulator(checker, sim_align_lib):
    import pileup_cases as pc
    res = xc.check_pipeline(ac.Goldens(), pc.Ctx(sim_align_lib, EX_PREFIX), checker)
    assert set(int(s) for s in res["status"]) <= {OK, REF_END}


# ------------------------------------------------------------------ 4. the adaptive band through model, training, pile-up and options
@pytest.fixture(scope="module")
def pipe(sim_align_lib):
    return apc.Ctx(sim_align_lib, EX_PREFIX)


@pytest.mark.lanesim
def test_pipeline_with_a_custom_model_under_the_emulator(pipe):
    apc.check_custom_model(pipe)


@pytest.mark.lanesim
@pytest.mark.parametrize("keep_shared", [False, True])
def test_training_with_an_open_end_under_the_emulator(pipe, keep_shared):
    apc.check_training(pipe, keep_shared)


@pytest.mark.lanesim
def test_pipeline_rounds_through_the_hook_under_the_emulator(pipe):
    apc.check_rounds(pipe)


@pytest.mark.lanesim
def test_pipeline_options_with_the_adaptive_band_under_the_emulator(pipe):
    apc.check_options(pipe)


@pytest.mark.lanesim
def test_a_path_without_a_start_in_the_pipeline_under_the_emulator(pipe):
    apc.check_left_band(pipe)
