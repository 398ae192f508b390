"""TEST INFRASTRUCTURE: the CPU checker of the banded DTW tests -- tests/dtw_band_check.c compiled on first use (gcc -O2
-ffp-contract=off) into a temporary directory.  tests/test_dtw_band_cpu.py anchors it on the reference's committed results
(tests/golden/dtw_goldens.npz); it stores O(cols * band) and so is the yardstick for long alignments too."""
import atexit
import ctypes as C
import shutil
import subprocess
import tempfile
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
OK, TOO_NARROW, LEFT_BAND = 0, 5, 6


def centre(j, rows, cols):
    return (np.asarray(j, np.uint64) * np.uint64(rows)) // np.uint64(cols)


def path_halfwidth(path, rows, cols):
    """the largest |i - c(j)| over a path of (event j, k-mer i) pairs: the narrowest band that holds it"""
    j, i = path[:, 0].astype(np.int64), path[:, 1].astype(np.int64)
    return int(np.abs(i - centre(j, rows, cols).astype(np.int64)).max())


def narrowest(rows, cols):
    """the smallest half-width that is feasible (W >= 1): ceil(rows / cols) <= W + 1"""
    return max(1, -(-rows // cols) - 1)


class BandChecker:
    _lib = None

    def __init__(self, model=None):
        """model: (means, vars_x2, lognorm) of the r9.4 template model, 1024 float32 each (default: the library's host tables)"""
        if BandChecker._lib is None:
            tmp = tempfile.mkdtemp(prefix="dtw_band_check_")
            atexit.register(shutil.rmtree, tmp, ignore_errors=True)
            so = Path(tmp) / "libdtw_band_check.so"
            subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", str(so), str(HERE / "dtw_band_check.c"), "-lm"],
                           check=True)
            L = C.CDLL(str(so))
            L.dtw_band_check.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_float, C.c_float,
                                         C.c_float, C.c_uint64, C.POINTER(C.c_float), C.POINTER(C.c_uint64), C.c_void_p,
                                         C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]
            BandChecker._lib = L
        if model is None:
            from uncalled_amd import capi
            model = capi.dtw_model_tables()
        self.model = np.ascontiguousarray(np.concatenate([np.asarray(m, np.float32) for m in model]))
        assert self.model.size == 3 * 1024

    def dtw(self, events, kmers, cost, dw, hw, vw, band):
        """-> score, score_bits, mean, path_len, path (end cell first, (event, k-mer) pairs), status (0, 5 or 6), ties"""
        ev = np.ascontiguousarray(events, np.float32)
        km = np.ascontiguousarray(kmers, np.uint16)
        path = np.empty((ev.size + km.size - 1, 2), np.uint32)
        score, n, status, ties = C.c_float(), C.c_uint64(), C.c_uint32(), C.c_uint64()
        rc = self._lib.dtw_band_check(ev.ctypes.data, ev.size, km.ctypes.data, km.size, self.model.ctypes.data, cost, dw, hw, vw, int(band),
                                      C.byref(score), C.byref(n), path.ctypes.data, C.byref(status), C.byref(ties))
        assert rc == 0
        s = np.float32(score.value)
        with np.errstate(all="ignore"):
            mean = np.float32(s / np.float32(n.value))
        return dict(score=s, score_bits=int(s.view(np.uint32)), mean=mean, path_len=int(n.value), path=path[:n.value].copy(),
                    status=int(status.value), ties=int(ties.value))
