"""CPU: the adaptive-band entry point exists wherever it must -- declared in include/uncalled_hip.h, exported by the gfx950 library
and by the emulator library of the tests, bound by capi and named with its status and its flag."""
import ctypes
import re

from conftest import ROOT, locked_make


def test_header_library_capi_and_emulator_hold_the_adaptive_entry_point():
    import __graft_entry__ as g
    from uncalled_amd import capi
    txt = (ROOT / "include" / "uncalled_hip.h").read_text()
    assert "UNC_DTW_REF_END 7u" in txt and "UNC_ALIGN_ADAPTIVE 16u" in txt
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert "unc_dtw_adapt_batch" in set(re.findall(r"\b(unc_[a-z0-9_]+)\s*\(", code))
    assert "k_dtw_adapt.hip" in g.HIP_INCLUDED
    L = ctypes.CDLL(str(g.build_hip()))          # hipcc cross-compiles for gfx950 without a GPU
    assert hasattr(L, "unc_dtw_adapt_batch")
    assert (capi.DTW_REF_END, capi.ALIGN_ADAPTIVE) == (7, 16)
    assert ctypes.sizeof(capi.AlignOpts) == 32 and capi.AlignOpts.band.offset == 28       # no field was added
    o = capi.align_opts(adaptive=128)
    assert (o.band, o.flags & capi.ALIGN_ADAPTIVE) == (128, 16) and capi.align_opts(band=7).flags & capi.ALIGN_ADAPTIVE == 0
    locked_make("-C", str(ROOT / "tests" / "lanesim"), "-f", "Makefile.dtw")
    sim = capi.load(ROOT / "tests" / "lanesim" / "_build_dtw" / "libuncalled_sim_dtw.so")
    assert hasattr(sim, "unc_dtw_adapt_batch") and sim.unc_dtw_adapt_batch.argtypes is not None
