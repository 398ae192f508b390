"""CPU: the pile-up's level histograms and the Kolmogorov-Smirnov kernel (k_pileup_hist.hip, unc_pileup_hist.cpp) below the GPU -- the
kernel sources and the host code under the lanesim emulator, against tests/pileup_hist_naive.py (Python integers and fractions).  The
cases are those of tests/test_gpu_pileup_hist.py.

The emulator library is built and copied exactly as the fixture of tests/test_pileup_cpu.py does it."""
import ctypes
import shutil
import subprocess

import pytest

import pileup_cases as pc
import pileup_hist_cases as hc
import refalign_cases as rc
import segments_cases as sc
from conftest import EX_PREFIX, ROOT, build_lock

SIM_DIR = ROOT / "tests" / "lanesim"
SIM_LIB = SIM_DIR / "_build_align" / "libuncalled_sim_align.so"


@pytest.fixture(scope="module")
def sim_align_path(tmp_path_factory):
    """a private copy of the emulator library, made after it was brought up to date with every source, included ones too"""
    import __graft_entry__ as g
    mine = tmp_path_factory.mktemp("sim_pileup_hist") / SIM_LIB.name
    with build_lock():
        sources = [g.CSRC / f for f in g.HIP_INCLUDED + g.HIP_SOURCES] + list(g.CSRC.glob("*.h"))
        stale = SIM_LIB.exists() and any(f.stat().st_mtime > SIM_LIB.stat().st_mtime for f in sources)
        subprocess.run(["make", "-s", "-C", str(SIM_DIR), "-f", "Makefile.align"] + (["-B"] if stale else []), check=True)
        assert all(f.stat().st_mtime <= SIM_LIB.stat().st_mtime for f in sources), "the emulator library is older than a source"
        shutil.copy2(SIM_LIB, mine)
    return mine


@pytest.fixture(scope="module")
def L(sim_align_path):
    from uncalled_amd import capi
    assert str(sim_align_path) not in capi._libs         # nobody can have opened this path before
    lib = capi.load(sim_align_path)
    assert hasattr(lib, "unc_pileup_hist_enable") and hasattr(lib, "unc_pileup_ks")
    return lib


@pytest.fixture(scope="module")
def X(L):
    return pc.Ctx(L, EX_PREFIX)


@pytest.fixture(scope="module")
def reads():
    return sc.Reads()


@pytest.fixture(scope="module")
def M(L, tmp_path_factory):
    prefix, seqs = rc.multi_reference(tmp_path_factory.mktemp("multi_hist"))
    ctx = pc.Ctx(L, prefix, seqs)
    assert ctx.lens == list(rc.MULTI_LENS) == [len(s) for s in seqs]
    return ctx


def test_included_sources_are_part_of_the_build():
    import __graft_entry__ as g
    assert "k_pileup_hist.hip" in g.HIP_INCLUDED and "unc_pileup_hist.cpp" in g.HIP_INCLUDED
    assert (g.CSRC / "k_align.hip").read_text().rstrip().endswith('#include "k_pileup_hist.hip"')
    assert '#include "unc_pileup_hist.cpp"' in (g.CSRC / "unc_align.cpp").read_text()
    assert "k_pileup_hist" not in (SIM_DIR / "Makefile.align").read_text()       # found through the includes


def test_layout_and_symbols(L):
    """8. under the emulator, and the gfx950 library, which hipcc cross-compiles without a GPU"""
    import __graft_entry__ as g
    hc.case_layout(L)
    hip = ctypes.CDLL(str(g.build_hip()))
    for name in hc.NAMES:
        assert hasattr(hip, name), name


def test_naive_checker_by_hand():
    """the checker itself on numbers worked out by hand.  Buckets: w = 4, c = 100: t = q - 100 + 128, so q = 100 is bucket 32, 99 is
    31, 103 is 32, 104 is 33, -28 is bucket 0 and so is everything below, 224 = 100 + 31 * 4 is bucket 63 and so is everything above.
    KS: rows (1, 1, 0, ...) and (0, 0, 2, 0, ...) are disjoint: d = 1; (1, 0, 1) against (0, 2, 0): the cumulative fractions are
    1/2, 1/2, 1 and 0, 1, 1: the distance 1/2 is reached at buckets 0 and 1, the lower wins, num = 1/2 * 2 * 2 = 2"""
    import math
    import pileup_hist_naive as hn
    assert [hn.bucket_of(q, 100, 4) for q in (100, 99, 103, 104, -28, -29, -10 ** 9, 224, 227, 228, 10 ** 9)] == [32, 31, 32, 33, 0, 0, 0, 63, 63, 63, 63]
    assert hn.centre_of(1.5) == 3 << 19 and hn.width_of(0.25) == 1 << 18 and hn.width_of(2048.0) == 1 << 31 and hn.width_of(2.0 ** -20) == 1
    assert hn.level_with_q(3 << 19) == 1.5 and hn.level_with_q(2 ** 27 + 1) is None and hn.level_with_q(2 ** 31) is None
    row = lambda *xs: list(xs) + [0] * (64 - len(xs))       # noqa: E731
    assert hn.ks(row(1, 1), row(0, 0, 2)) == (2, 2, 4, 1, 1, 1.0, 1.0)
    assert hn.ks(row(0, 0, 2), row(1, 1)) == (2, 2, 4, 1, -1, 1.0, 1.0)
    assert hn.ks(row(1, 0, 1), row(0, 2, 0)) == (2, 2, 2, 0, 1, 0.5, 0.5)
    assert hn.ks(row(3, 1), row(3, 1)) == (4, 4, 0, 0, 0, 0.0, 0.0)
    n_a, n_b, num, bucket, sign, d, ks = hn.ks(row(1, 2), row(0, 1))
    assert (n_a, n_b, num, bucket, sign) == (3, 1, 1, 0, 1) and d == 1.0 / 3.0 and ks == d * math.sqrt(3.0 / 4.0)
    h = hn.Hist([(0, 10, 20)], lambda key: 100, 4).add([0, 0, 0, 0], [10, 10, 10, 16], [1, 1, 0, 1], [100 / 2 ** 20, 104 / 2 ** 20, 0.0, 1.0], [1] * 4)
    assert h.rows == {(0, 10, 0): row(*[0] * 32, 1, 1), (0, 10, 1): row(*[0] * 7, 1)} and h.nv.counters() == (0, 1, 3)


@pytest.mark.lanesim
def test_centres(X):
    hc.case_centres(X)


@pytest.mark.lanesim
def test_centres_sequences(M):
    hc.case_centres_sequences(M)


@pytest.mark.lanesim
def test_bucket_edges(X):
    hc.case_bucket_edges(X)


@pytest.mark.lanesim
def test_one_bin_many_workgroups(X):
    hc.case_one_bin(X)


@pytest.mark.lanesim
def test_order_split_reset(X):
    hc.case_order_split_reset(X)


@pytest.mark.lanesim
def test_merge(X):
    hc.case_merge(X)


@pytest.mark.lanesim
def test_enable_refusals(X):
    hc.case_enable_refusals(X)


@pytest.mark.lanesim
def test_through_the_alignment(X, reads):
    hc.case_through_the_alignment(X, reads)


@pytest.mark.lanesim
def test_ks(X):
    hc.case_ks(X)


@pytest.mark.lanesim
def test_ks_wide_and_refusals(X):
    hc.case_ks_wide_and_refusals(X)
