"""TEST INFRASTRUCTURE: the CPU checker of the adaptive-band DTW tests -- tests/dtw_adapt_check.c compiled on first use (gcc -O2
-ffp-contract=off) into a temporary directory.  AdaptChecker.dtw is the adaptive band with an open end exactly as
include/uncalled_hip.h states it, AdaptChecker.full the full matrix with the same recurrence and the same end scan;
tests/test_dtw_adapt_cpu.py anchors both on tests/dtw_check.c and the reference's committed results."""
import atexit
import ctypes as C
import shutil
import subprocess
import tempfile
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
OK, LEFT_BAND, REF_END = 0, 6, 7
BANDS = (64, 128, 256)


def adapt_crumb_bytes(rows, cols, band):
    """bytes of back-pointers and lo_d the library holds for one adaptive alignment (dtw_adapt_words of dtw_dev.h, times 4)"""
    n = rows + cols - 1
    return 4 * ((n + 15) // 16 * band + (n + 63) // 64 * 64)


class AdaptChecker:
    _lib = None

    def __init__(self, model=None):
        """model: (means, vars_x2, lognorm) of the r9.4 template model, 1024 float32 each (default: the library's host tables)"""
        if AdaptChecker._lib is None:
            tmp = tempfile.mkdtemp(prefix="dtw_adapt_check_")
            atexit.register(shutil.rmtree, tmp, ignore_errors=True)
            so = Path(tmp) / "libdtw_adapt_check.so"
            subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", str(so), str(HERE / "dtw_adapt_check.c"), "-lm"],
                           check=True)
            L = C.CDLL(str(so))
            f, u64, vp = C.c_float, C.c_uint64, C.c_void_p
            L.dtw_adapt_check.argtypes = [vp, u64, vp, u64, vp, C.c_uint32, f, f, f, u64, C.POINTER(f), C.POINTER(u64), vp,
                                          C.POINTER(C.c_uint32), vp, C.POINTER(u64), vp, C.POINTER(C.c_uint32)]
            L.dtw_open_check.argtypes = [vp, u64, vp, u64, vp, C.c_uint32, f, f, f, C.POINTER(f), C.POINTER(u64), vp, C.POINTER(C.c_uint32), vp]
            AdaptChecker._lib = L
        if model is None:
            from uncalled_amd import capi
            model = capi.dtw_model_tables()
        self.model = np.ascontiguousarray(np.concatenate([np.asarray(m, np.float32) for m in model]))
        assert self.model.size == 3 * 1024

    @staticmethod
    def _out(score, n, path, status, end_row, **more):
        s = np.float32(score.value)
        with np.errstate(all="ignore"):
            mean = np.float32(s / np.float32(n.value))
        return dict(score=s, score_bits=int(s.view(np.uint32)), mean=mean, path_len=int(n.value), path=path[:n.value].copy(),
                    status=int(status), end_row=None if end_row.value == 0xFFFFFFFF else int(end_row.value), **more)

    def dtw(self, events, kmers, cost, dw, hw, vw, band, cells=False):
        """the adaptive band -> score, score_bits, mean, path_len, path (end cell first, (event, k-mer) pairs), status (0, 6 or 7),
        end_row (None: no cell of the last column was computed), lo (lo_d of the anti-diagonals computed); cells=True: also
        `cells`, a dict (i, j) -> score of every computed cell"""
        assert band in BANDS
        ev = np.ascontiguousarray(events, np.float32)
        km = np.ascontiguousarray(kmers, np.uint16)
        n_diag = ev.size + km.size - 1
        path = np.empty((n_diag, 2), np.uint32)
        lo = np.zeros(n_diag, np.int32)
        grid = np.full((n_diag, band), np.nan, np.float32) if cells else None
        score, n, status, n_done, end_row = C.c_float(), C.c_uint64(), C.c_uint32(), C.c_uint64(), C.c_uint32()
        rc = self._lib.dtw_adapt_check(ev.ctypes.data, ev.size, km.ctypes.data, km.size, self.model.ctypes.data, cost, dw, hw, vw, int(band),
                                       C.byref(score), C.byref(n), path.ctypes.data, C.byref(status), lo.ctypes.data, C.byref(n_done),
                                       grid.ctypes.data if cells else None, C.byref(end_row))
        assert rc == 0
        more = dict(lo=lo[:n_done.value].copy())
        if cells:
            got = {}
            for d in range(int(n_done.value)):
                it = max(int(lo[d]), 0, d - (ev.size - 1))
                ib = min(int(lo[d]) + band - 1, km.size - 1, d)
                for i in range(it, ib + 1):
                    got[(i, d - i)] = grid[d, i - int(lo[d])]
            more["cells"] = got
        return self._out(score, n, path, status.value, end_row, **more)

    def full(self, events, kmers, cost, dw, hw, vw, cells=False):
        """the full matrix with the open end -> as dtw(), status 0 or 7; cells=True: also `cells`, the rows x cols scores"""
        ev = np.ascontiguousarray(events, np.float32)
        km = np.ascontiguousarray(kmers, np.uint16)
        path = np.empty((ev.size + km.size - 1, 2), np.uint32)
        grid = np.empty((km.size, ev.size), np.float32) if cells else None
        score, n, end_row = C.c_float(), C.c_uint64(), C.c_uint32()
        rc = self._lib.dtw_open_check(ev.ctypes.data, ev.size, km.ctypes.data, km.size, self.model.ctypes.data, cost, dw, hw, vw,
                                      C.byref(score), C.byref(n), path.ctypes.data, C.byref(end_row), grid.ctypes.data if cells else None)
        assert rc == 0
        return self._out(score, n, path, REF_END if end_row.value == km.size - 1 else OK, end_row, **(dict(cells=grid) if cells else {}))
