"""CPU: the signal pile-up (k_pileup.hip, unc_pileup.cpp) below the GPU -- the kernel sources and the host code under the lanesim
emulator, against tests/pileup_naive.py (Python integers).  The cases are those of tests/test_gpu_pileup.py.

The emulator library is the one tests/lanesim/Makefile.align builds; as in tests/test_model_cpu.py the fixture rebuilds it when it
is older than a source (included ones too, which the make file does not know) and loads a COPY under a path of its own."""
import shutil
import subprocess

import pytest

import pileup_cases as pc
import refalign_cases as rc
import segments_cases as sc
from conftest import EX_PREFIX, ROOT, build_lock

SIM_DIR = ROOT / "tests" / "lanesim"
SIM_LIB = SIM_DIR / "_build_align" / "libuncalled_sim_align.so"


@pytest.fixture(scope="module")
def sim_align_path(tmp_path_factory):
    """a private copy of the emulator library, made after it was brought up to date with every source, included ones too"""
    import __graft_entry__ as g
    mine = tmp_path_factory.mktemp("sim_pileup") / SIM_LIB.name
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
    assert hasattr(lib, "unc_pileup_create") and hasattr(lib, "unc_align_pileup_call")
    return lib


@pytest.fixture(scope="module")
def X(L):
    return pc.Ctx(L, EX_PREFIX)


@pytest.fixture(scope="module")
def reads():
    return sc.Reads()


@pytest.fixture(scope="module")
def M(L, tmp_path_factory):
    """five sequences; the default table must keep k_pileup_scan at three passes"""
    prefix, seqs = rc.multi_reference(tmp_path_factory.mktemp("multi"))
    ctx = pc.Ctx(L, prefix, seqs)
    assert ctx.lens == list(rc.MULTI_LENS) == [len(s) for s in seqs]
    n_bins = ctx.pileup().n_bins()
    assert n_bins == 528106 and -(-n_bins // pc.SCAN_CHUNK) == 516
    return ctx


def test_included_sources_are_part_of_the_build():
    import __graft_entry__ as g
    assert "k_pileup.hip" in g.HIP_INCLUDED and "unc_pileup.cpp" in g.HIP_INCLUDED
    assert '#include "k_pileup.hip"' in (g.CSRC / "k_align.hip").read_text()
    assert '#include "unc_pileup.cpp"' in (g.CSRC / "unc_align.cpp").read_text()


def test_layout_and_symbols(L):
    pc.case_layout(L)


def test_naive_checker_by_hand():
    """the checker itself on numbers worked out by hand: q of 1.5 is 1.5 * 2^20; two records of 1.5 and 2.5 have mean 2, sd 0.5"""
    import math
    import pileup_naive as pn
    nv = pn.Naive([(0, 10, 20)]).add([0, 0, 0], [10, 10, 16], [1, 1, 1], [1.5, 2.5, 3.0], [4, 6, 1])
    assert nv.bins == {(0, 10, 0): [2, 4 << 20, (9 << 38) + (25 << 38), 10]} and nv.counters() == (0, 1, 2)
    assert pn.stats(nv.bins[(0, 10, 0)], 1.0, 0.5)[1:] == (2.0, 0.5, 5.0, 2.0 * math.sqrt(2.0))
    assert pn.py_kmer("ACGTAC", 0, True) == 0b0001101100 and pn.py_kmer("ACGTAC", 1, False) == pn.py_kmer("GTACG", 0, True)
    assert nv.keys_in_order()[:3] == [(0, 10, 0), (0, 10, 1), (0, 11, 0)] and len(nv.keys_in_order()) == 12
    # two sequences, given unsorted: sequence 0 has positions 3 and 4, sequence 1 positions 0..2 and a region of 4 bases without a bin
    two = pn.Naive([(1, 0, 7), (1, 20, 24), (0, 3, 9)])
    assert two.keys_in_order() == [(0, 3, 0), (0, 3, 1), (0, 4, 0), (0, 4, 1), (1, 0, 0), (1, 0, 1), (1, 1, 0), (1, 1, 1), (1, 2, 0), (1, 2, 1)]
    two.add([1, 0, 0, 1, 1, 1, 0], [0, 4, 5, 3, 20, 2, 4], [1, 0, 1, 1, 1, 0, 0], [1.0] * 7, [2] * 7)
    assert two.bins == {(1, 0, 0): [1, 1 << 20, 1 << 40, 2], (0, 4, 1): [2, 2 << 20, 2 << 40, 4], (1, 2, 1): [1, 1 << 20, 1 << 40, 2]}
    assert two.counters() == (0, 3, 4)      # (0, 5), (1, 3) and (1, 20) hold no whole k-mer of their regions
    assert two.covered(1) == [3, 4, 9] == two.covered_of_bins(1) and two.covered(2) == [3] == two.covered_of_bins(2)
    assert two.covered(1, pn.Naive(two.regions).add([1], [2], [0], [1.0], [1])) == [9] == two.covered_of_bins(1, pn.Naive(two.regions).add([1], [2], [0], [1.0], [1]))
    assert [two.bin_of(k) for k in two.keys_in_order()] == list(range(10)) and [two.key_of(i) for i in range(10)] == two.keys_in_order()
    for bad in ((1, 3, 0), (0, 2, 0), (1, 20, 0), (2, 0, 0)):
        with pytest.raises(KeyError):
            two.bin_of(bad)


@pytest.mark.lanesim
def test_one_bin_many_workgroups(X):
    pc.case_one_bin(X)


@pytest.mark.lanesim
def test_carry_and_sign(X):
    pc.case_carry(X)


@pytest.mark.lanesim
def test_dropped_skipped_outside(X):
    pc.case_dropped_skipped_outside(X)


@pytest.mark.lanesim
def test_strands(X):
    pc.case_strands(X)


@pytest.mark.lanesim
def test_order_and_split(X):
    pc.case_order_and_split(X)


@pytest.mark.lanesim
def test_regions(X):
    pc.case_regions(X)


@pytest.mark.lanesim
def test_through_the_alignment(X, reads):
    pc.case_through_the_alignment(X, reads)


@pytest.mark.lanesim
def test_with_an_accumulator(X, reads):
    pc.case_with_an_accumulator(X, reads)


@pytest.mark.lanesim
def test_covered(X):
    pc.case_covered(X)


@pytest.mark.lanesim
def test_stats_and_compare(X):
    pc.case_stats_and_compare(X)


@pytest.mark.lanesim
def test_merge(X):
    pc.case_merge(X)


@pytest.mark.lanesim
def test_refusals(X, reads):
    pc.case_refusals(X, reads)


@pytest.mark.lanesim
def test_sequences(M):
    pc.case_sequences(M)


@pytest.mark.lanesim
def test_stats_sequences(M):
    pc.case_stats_sequences(M)


@pytest.mark.lanesim
@pytest.mark.parametrize("fill", ["a", "b", "c", "d", "e"])
def test_scan_passes(M, fill):
    pc.case_scan_passes(M, fill)


@pytest.mark.lanesim
def test_scan_merge_gather(M):
    pc.case_scan_merge_gather(M)


@pytest.mark.lanesim
def test_alignment_sequences(M, reads):
    pc.case_alignment_sequences(M, reads)


@pytest.mark.lanesim
def test_alignment_sequences_band_and_cut(M, reads):
    pc.case_alignment_sequences_band_and_cut(M, reads)


@pytest.mark.lanesim
def test_alignment_sequences_accumulator_and_regions(M, reads):
    pc.case_alignment_sequences_accumulator_and_regions(M, reads)
