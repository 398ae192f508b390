"""GPU: the leaf bench on the MI355X -- the cases of tests/leaves_cases.py (the same ones tests/test_leaves_cpu.py runs under the
emulator) through the gfx950 build of tests/leaves/k_leaves.hip, compared for exact equality with tests/leaves_naive.py.  A family is
one launch, a workgroup per case."""
import pytest

import leaves_cases as lc
import leaves_lib

PATTERNS, PATTERNS128 = lc.PATTERNS, lc.PATTERNS128

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    return leaves_lib.hip()      # (no library and no hipcc: an error, not a skip)


@pytest.mark.parametrize("bits", [64, 32])
def test_segmented_max_scans(bits, L):
    lc.check_seg_scans(L, bits)


def test_wave_sums_maxima_and_popcounts(L):
    lc.check_wave_sums(L)


def test_wave_broadcasts(L):
    lc.check_wave_bcasts(L)


@pytest.mark.parametrize("pattern", PATTERNS)
def test_sort_any64(pattern, L):
    lc.check_sort64(L, pattern)


def test_sort_any64_in_place_with_exactly_n_keys_of_room(L):
    lc.check_sort64_in_place(L)


def test_sort64_size_classes_by_name(L):
    lc.check_sort64_classes(L)


@pytest.mark.parametrize("pattern", PATTERNS128)
def test_legacy_sort128(pattern, L):
    lc.check_sort128(L, pattern)


def test_legacy_sort128_size_classes_by_name(L):
    lc.check_sort128_classes(L)


@pytest.mark.parametrize("kind", ["41", "14", "w41"])
def test_merge_runs(kind, L):
    lc.check_merge(L, kind)


def test_merge_runs_checks_its_own_output(L):
    lc.check_merge_verify(L)


def test_merge_splits_alone(L):
    lc.check_splits(L)


def test_staged_tiles(L):
    lc.check_tiles(L)


@pytest.mark.parametrize("wide", [False, True], ids=["narrow", "wide"])
def test_repair_run(wide, L):
    lc.check_repair_run(L, wide)


def test_repair_runs4(L):
    lc.check_repair_runs4(L)


@pytest.mark.parametrize("wide", [False, True], ids=["narrow", "wide"])
def test_phase_s_chain_at_the_leaf_level(wide, L):
    lc.check_chain(L, wide)
