"""TEST INFRASTRUCTURE: the two builds of the leaf bench (tests/leaves/k_leaves.hip) and the one call both export.  A helper, not a
conftest: tests/test_leaves_cpu.py and tests/test_gpu_leaves.py make their fixtures from it.

  sim()   tests/lanesim/Makefile.leaves -> tests/lanesim/_build_leaves/libunc_leaves_sim.so   (the emulator)
  hip()   hipcc, __graft_entry__'s compiler and flags -> tests/leaves/_build/libunc_leaves.so   (gfx950), rebuilt when older than
          its sources.  Without hipcc an existing library is used as it is; neither a library nor hipcc is an error.
"""
import ctypes
import os
import subprocess

import numpy as np

from conftest import ROOT, build_lock, locked_make

SRC = ROOT / "tests" / "leaves" / "k_leaves.hip"
CSRC = ROOT / "uncalled_amd" / "csrc"
HIP_LIB = ROOT / "tests" / "leaves" / "_build" / "libunc_leaves.so"
SIM_LIB = ROOT / "tests" / "lanesim" / "_build_leaves" / "libunc_leaves_sim.so"


class Leaves:
    """leaves_run of one build: run(kernel, desc, slots) launches len(desc) workgroups and hands descriptors and slots back."""

    def __init__(self, path):
        self.path = path
        self.lib = ctypes.CDLL(str(path))
        self.lib.leaves_run.restype = ctypes.c_int
        self.lib.leaves_run.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint64]

    def run(self, kernel, desc, slots):
        """desc: uint32 [ncases, 32]; slots: uint8 [ncases, slot_bytes].  Both are copies on return; the arguments stay as they were."""
        desc = np.ascontiguousarray(desc, dtype=np.uint32).copy()
        slots = np.ascontiguousarray(slots, dtype=np.uint8).copy()
        assert desc.ndim == 2 and desc.shape[1] == 32 and slots.ndim == 2 and slots.shape[0] == desc.shape[0] and slots.shape[1] % 16 == 0
        err = self.lib.leaves_run(int(kernel), desc.ctypes.data, desc.shape[0], slots.ctypes.data, slots.shape[1])
        assert err != -2, "leaves_run(kernel %d): the launch wrote behind its last slot" % kernel
        assert err == 0, "leaves_run(kernel %d): error %d" % (kernel, err)
        return desc, slots


def sim():
    alt = os.environ.get("UNC_LEAVES_CSRC")      # dev: the bench over another copy of the kernel headers (a seeded fault), always rebuilt
    if alt:
        locked_make("-B", "-C", str(ROOT / "tests" / "lanesim"), "-f", "Makefile.leaves", "CSRC=" + alt, "OUT=_build_leaves_alt")
        return Leaves(ROOT / "tests" / "lanesim" / "_build_leaves_alt" / "libunc_leaves_sim.so")
    locked_make("-C", str(ROOT / "tests" / "lanesim"), "-f", "Makefile.leaves")
    return Leaves(SIM_LIB)


def hip():
    import __graft_entry__ as g
    deps = [SRC, ROOT / "include" / "uncalled_hip.h"] + list(CSRC.glob("*.h"))
    with build_lock():
        if g._stale(HIP_LIB, deps):
            try:
                cc = g._hipcc()
            except Exception:
                cc = None
            if cc:
                HIP_LIB.parent.mkdir(parents=True, exist_ok=True)
                subprocess.run([cc] + g.HIPCC_FLAGS + ["-I", str(CSRC), str(SRC), "-o", str(HIP_LIB)], check=True)
            elif not HIP_LIB.exists():
                raise RuntimeError("no hipcc and no prebuilt %s" % HIP_LIB)
    return Leaves(HIP_LIB)
