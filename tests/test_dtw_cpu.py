"""CPU: the DTW feature below the GPU -- the checker (tests/dtw_check.c) against the committed reference results, the C ABI's
declarations and exports, BwaIndex::get_kmers on the example index, and k_dtw.hip itself under the lanesim emulator (built by
tests/lanesim/Makefile.dtw, a make file of its own: the emulator suite's library does not hold the DTW sources)."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

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
