"""CPU: the leaf bench under the emulator -- k_map's sort, merge and repair leaves (map_sort.h, map_sort_wide.h) and the wave primitives
(wave_prims.h), each called alone by a thin kernel of tests/leaves/k_leaves.hip on inputs the cases of tests/leaves_cases.py chose,
and compared for exact equality with tests/leaves_naive.py.  tests/test_gpu_leaves.py runs the same cases on the MI355X."""
import numpy as np
import pytest

import leaves_cases as lc
import leaves_lib
import leaves_naive as ln

PATTERNS, PATTERNS128 = lc.PATTERNS, lc.PATTERNS128


@pytest.fixture(scope="module")
def L():
    return leaves_lib.sim()


def test_references_on_cases_worked_by_hand():
    """the plain references themselves, on inputs small enough to state the answer"""
    assert ln.repair([10, 100, 20, 30, 100, 101, 5]) == ([0, 1, 4, 5], [2, 3, 6])          # an equal key stays; 30 > 20 but < 100
    assert ln.repair([]) == ([], []) and ln.repair([7]) == ([0], [])
    assert ln.repair([(1, 5), (1, 4), (1, 5), (2, 0)], ln.wk_lt) == ([0, 2, 3], [1])
    h = np.zeros(64, dtype=np.uint32)
    h[[3, 16]] = 1
    v = np.arange(64, 0, -1).astype(np.uint64)
    s = ln.seg_incl_max(v, h)
    assert s[:3].tolist() == [64, 64, 64] and s[3:16].tolist() == [61] * 13 and s[16:].tolist() == [48] * 48
    pre, tot = ln.excl_sum(np.full(64, 1 << 31, dtype=np.uint64))
    assert pre[:4].tolist() == [0, 1 << 31, 0, 1 << 31] and tot == 0
    assert ln.prefix_popc(0b1011)[:5].tolist() == [0, 1, 2, 2, 3] and ln.wave_sum64(np.full(64, 1 << 58, dtype=np.uint64)) == 0
    assert ln.split(np.array([1, 4, 9]), np.array([2, 3, 10]), 4) == 2 and ln.split(np.array([5]), np.array([1]), 1) == 0
    k = np.array([[2, 1], [1, 9], [2, 0], [1, 3]], dtype=np.uint64)
    assert ln.sort128(k).tolist() == ln.sort128(k, legacy=True).tolist() == [[1, 3], [1, 9], [2, 0], [2, 1]]
    assert ln.key_gt((1, 2), (1, 1)) and not ln.key_gt((1, 1), (1, 1)) and ln.key_gt((2, 0), (1, 9))


@pytest.mark.lanesim
@pytest.mark.parametrize("bits", [64, 32])
def test_segmented_max_scans(bits, L):
    lc.check_seg_scans(L, bits)


@pytest.mark.lanesim
def test_wave_sums_maxima_and_popcounts(L):
    lc.check_wave_sums(L)


@pytest.mark.lanesim
def test_wave_broadcasts(L):
    lc.check_wave_bcasts(L)


@pytest.mark.lanesim
@pytest.mark.parametrize("pattern", PATTERNS)
def test_sort_any64(pattern, L):
    lc.check_sort64(L, pattern)


@pytest.mark.lanesim
def test_sort_any64_in_place_with_exactly_n_keys_of_room(L):
    lc.check_sort64_in_place(L)


@pytest.mark.lanesim
def test_sort64_size_classes_by_name(L):
    lc.check_sort64_classes(L)


@pytest.mark.lanesim
@pytest.mark.parametrize("pattern", PATTERNS128)
def test_legacy_sort128(pattern, L):
    lc.check_sort128(L, pattern)


@pytest.mark.lanesim
def test_legacy_sort128_size_classes_by_name(L):
    lc.check_sort128_classes(L)


@pytest.mark.lanesim
@pytest.mark.parametrize("kind", ["41", "14", "w41"])
def test_merge_runs(kind, L):
    lc.check_merge(L, kind)


@pytest.mark.lanesim
def test_merge_runs_checks_its_own_output(L):
    lc.check_merge_verify(L)


@pytest.mark.lanesim
def test_merge_splits_alone(L):
    lc.check_splits(L)


@pytest.mark.lanesim
def test_staged_tiles(L):
    lc.check_tiles(L)


@pytest.mark.lanesim
@pytest.mark.parametrize("wide", [False, True], ids=["narrow", "wide"])
def test_repair_run(wide, L):
    lc.check_repair_run(L, wide)


@pytest.mark.lanesim
def test_repair_runs4(L):
    lc.check_repair_runs4(L)


@pytest.mark.lanesim
@pytest.mark.parametrize("wide", [False, True], ids=["narrow", "wide"])
def test_phase_s_chain_at_the_leaf_level(wide, L):
    lc.check_chain(L, wide)
