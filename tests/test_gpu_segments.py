"""GPU: alignments in sample coordinates on the MI355X -- the cases of tests/segments_cases.py (shared with the emulator run of
tests/test_segments_cpu.py) through the gfx950 library: every record, info and tapped event against the checker chain in bits,
results, levels and paths against the entry points without segments byte for byte.  Slices of at most 3 000 samples: a case
takes well under a second of GPU time."""
import numpy as np
import pytest

import align_cases as ac
import segments_cases as sc
from conftest import EX_PREFIX

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def chain(oracle_lib):
    return sc.Chain(oracle_lib)


@pytest.fixture(scope="module")
def reads():
    return sc.Reads()


@pytest.mark.parametrize("name", list(sc.CASES))
def test_case(name, chain, hip_lib, reads):
    assert hasattr(hip_lib, "unc_align_segments_batch")
    sc.CASES[name](chain, hip_lib, reads)


def test_goldens_unchanged_through_the_new_entry_point(hip_lib):
    G = ac.Goldens()
    assert sc.check_goldens_unchanged(G, hip_lib) == G.n


def test_example_read_by_coordinates_and_by_kmers(chain, hip_lib):
    from uncalled_amd import capi
    G = ac.Goldens()
    ix = capi.Index(EX_PREFIX)
    rs = capi.RefSeq(ix, EX_PREFIX)
    segs, kms = sc.check_example(chain, G, rs, ix, str(EX_PREFIX))
    assert segs[0].size == kms[0].size == 296 and segs[1].size == 296
    # the binding, by coordinates: the same records
    r = len(G.signals) - 1
    out = capi.align_ref_batch(rs, G.raw, G.offsets, G.calib, [(r, 10001, 14001)] * 2, [(0, 6700, 7000, True), (0, 6700, 7000, False)],
                               segments=True, events=True)
    assert all(sc.rec_equal(x, y) for x, y in zip(out[1], segs)) and [int(x) for x in out[2]["n_rows"]] == [296, 296]
    assert capi.align_segments_last_timing() > 0
    sc.check_ref_argument_errors(G, rs)
    rs.close()


def test_binding_order_by_coordinates_and_by_kmers(hip_lib):
    from uncalled_amd import capi
    ix = capi.Index(EX_PREFIX)
    rs = capi.RefSeq(ix, EX_PREFIX)
    sc.check_binding_order(ac.Goldens(), rs, ix, str(EX_PREFIX))
    rs.close()


def test_the_stage_is_timed(hip_lib, reads):
    from uncalled_amd import capi
    capi.align_batch(reads.raw, reads.offsets, reads.calib, [(0, 0, 2000)], [reads.walk[:200]])
    assert capi.align_segments_last_timing() == 0           # a call without segments
    capi.align_batch(reads.raw, reads.offsets, reads.calib, [(0, 0, 2000)], [reads.walk[:200]], segments=True)
    assert capi.align_segments_last_timing() > 0 and np.isfinite(capi.align_last_timing()).all()
