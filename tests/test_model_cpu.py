"""CPU: the pore model object, the training accumulator (k_model.hip) and the model in the alignment, below the GPU -- the kernel
sources and the host code under the lanesim emulator, against tests/model_naive.py (Python integers), tests/model_check.c and the
checker chain of tests/segments_cases.py built for the model under test.  The cases are those of tests/test_gpu_model.py.

The emulator library is the one tests/lanesim/Makefile.align builds.  That make file does not know the sources its sources include
(k_model.hip, unc_model.cpp and unc_model_acc.cpp among them), and capi.load() keeps one handle per path for the life of the process, so the fixture
below rebuilds the library when it is older than an included source and loads a COPY of the file under a path of its own."""
import shutil
import subprocess

import pytest

import model_cases as mc
import segments_cases as sc
from conftest import EX_PREFIX, ROOT, build_lock

SIM_DIR = ROOT / "tests" / "lanesim"
SIM_LIB = SIM_DIR / "_build_align" / "libuncalled_sim_align.so"


@pytest.fixture(scope="module")
def sim_align_path(tmp_path_factory):
    """a private copy of the emulator library, made after it was brought up to date with every source, included ones too"""
    import __graft_entry__ as g
    mine = tmp_path_factory.mktemp("sim_model") / SIM_LIB.name
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
    assert hasattr(lib, "unc_model_load") and hasattr(lib, "unc_model_acc_add") and hasattr(lib, "unc_align_call")
    return lib


@pytest.fixture(scope="module")
def reads():
    return sc.Reads()


def test_included_sources_are_part_of_the_build():
    import __graft_entry__ as g
    assert "k_model.hip" in g.HIP_INCLUDED and "unc_model.cpp" in g.HIP_INCLUDED
    assert '#include "k_model.hip"' in (g.CSRC / "k_align.hip").read_text()
    assert "unc_model_acc.cpp" in g.HIP_INCLUDED and '#include "unc_model_acc.cpp"' in (g.CSRC / "unc_align.cpp").read_text()
    assert '#include "unc_model.cpp"' in (g.CSRC / "unc_host.cpp").read_text()


def test_record_layout():
    import ctypes
    from uncalled_amd import capi
    assert ctypes.sizeof(capi.AlignCall) == 200 and capi.AlignCall.accumulate.offset == 184 and capi.AlignCall.queries.offset == 64


# ---- the model object: no device
def test_default_pairs(L):
    mc.case_default_pairs(L)


@pytest.mark.lanesim
def test_default_tables_are_the_index_s_and_the_dtw_s(L):
    from uncalled_amd import capi
    mc.case_default_tables(L, capi.Index(EX_PREFIX, lib=L))


def test_save_load_round_trip_and_shuffled_order(L, tmp_path):
    mc.case_round_trip(L, tmp_path)


def test_malformed_files_are_refused(L, tmp_path):
    mc.case_malformed(L, tmp_path)


def test_random_tables_against_model_check(L):
    mc.case_random_tables(L)


# ---- the accumulator through acc_add
@pytest.mark.lanesim
def test_acc_one_bin_two_workgroups(L):
    mc.case_one_bin(L)


@pytest.mark.lanesim
def test_acc_carry_into_the_high_word(L):
    mc.case_carry(L)


@pytest.mark.lanesim
def test_acc_dropped_and_skipped(L):
    mc.case_drop_and_skip(L)


@pytest.mark.lanesim
def test_acc_split_and_order(L):
    mc.case_split_and_order(L)


@pytest.mark.lanesim
def test_acc_finish(L):
    mc.case_finish(L)


# ---- through the alignment
@pytest.mark.lanesim
def test_align_accumulates(L, reads):
    mc.case_align_accumulates(L, reads)


@pytest.mark.lanesim
def test_align_short_room(L, reads):
    mc.case_align_short_room(L, reads)


@pytest.mark.lanesim
def test_default_model_changes_nothing(L, reads):
    mc.case_default_model_changes_nothing(L, reads)


@pytest.mark.lanesim
def test_random_model_alignment(L, reads, oracle_lib):
    mc.case_random_model_alignment(L, reads, oracle_lib)


@pytest.mark.lanesim
def test_dtw_model_batch(L):
    mc.case_dtw_model_batch(L)
