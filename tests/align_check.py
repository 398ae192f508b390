"""TEST INFRASTRUCTURE: the CPU checker of the alignment tests -- tests/align_check.c compiled on first use (gcc -O2
-ffp-contract=off) into a temporary directory.  It reproduces every case of tests/golden/align_goldens.npz bit for bit
(tests/test_align_cpu.py) and, chained between the event detector's restatement and tests/dtw_check.c, is the yardstick for shapes
the goldens do not hold (expected())."""
import atexit
import ctypes as C
import shutil
import subprocess
import tempfile
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent


class AlignChecker:
    _lib = None

    def __init__(self, model_means=None):
        if AlignChecker._lib is None:
            tmp = tempfile.mkdtemp(prefix="align_check_")
            atexit.register(shutil.rmtree, tmp, ignore_errors=True)
            so = Path(tmp) / "libalign_check.so"
            subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", str(so), str(HERE / "align_check.c"), "-lm"], check=True)
            L = C.CDLL(str(so))
            L.align_check_mask.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
            L.align_check_mask.restype = C.c_uint32
            L.align_check_target.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_float), C.POINTER(C.c_float)]
            L.align_check_normalize.argtypes = [C.c_void_p, C.c_uint32, C.c_float, C.c_float, C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float)]
            AlignChecker._lib = L
        if model_means is None:
            from uncalled_amd import capi
            model_means = capi.dtw_model_tables()[0]
        self.means = np.ascontiguousarray(model_means, np.float32)
        assert self.means.size == 1024

    def mask(self, event_means):
        ev = np.ascontiguousarray(event_means, np.float32)
        m = np.zeros(max(1, ev.size), np.uint8)
        kept = self._lib.align_check_mask(ev.ctypes.data, ev.size, m.ctypes.data)
        m = m[:ev.size].astype(bool)
        assert kept == int(m.sum())
        return m

    def target(self, kmers):
        km = np.ascontiguousarray(kmers, np.uint16)
        a, b = C.c_float(), C.c_float()
        self._lib.align_check_target(self.means.ctypes.data, km.ctypes.data, km.size, C.byref(a), C.byref(b))
        return np.float32(a.value), np.float32(b.value)

    def normalize(self, x, tgt_mean, tgt_stdv):
        """-> levels, scale, shift"""
        x = np.ascontiguousarray(x, np.float32)
        out = np.empty(max(1, x.size), np.float32)
        a, b = C.c_float(), C.c_float()
        self._lib.align_check_normalize(x.ctypes.data, x.size, C.c_float(float(tgt_mean)), C.c_float(float(tgt_stdv)), out.ctypes.data,
                                        C.byref(a), C.byref(b))
        return out[:x.size], np.float32(a.value), np.float32(b.value)

    def stages(self, columns, kmers, mask=True, target="kmers", model_target=None):
        """stages b to d over the kept event means (or the calibrated samples, with mask=False) of one query"""
        x = np.ascontiguousarray(columns, np.float32)
        m = self.mask(x) if mask else np.ones(x.size, bool)
        tm, ts = self.target(kmers) if target == "kmers" else model_target
        kept = x[m]
        if kept.size:
            lev, scale, shift = self.normalize(kept, tm, ts)
        else:
            lev, scale, shift = kept, np.float32(0), np.float32(0)
        return dict(mask=m, tgt_mean=np.float32(tm), tgt_stdv=np.float32(ts), scale=scale, shift=shift, levels=lev)


def expected(po, ac, dc, signal_i16, calib, query, kmers, mask=True, create_events=True, target="kmers", model_target=None, dtw=(0, 1, 1.0, 1.0, 1.0)):
    """The checker chain for one query: calibration and event detection of the slice by the detector's restatement (po =
    oracle.pyoracle), stages b to d by ac (AlignChecker), the DTW by dc (dtw_check.Checker).  calib = (range, offset, digitisation),
    query = (smp_st, smp_en), dtw = (subseq, cost, dw, hw, vw)."""
    st, en = query
    en = len(signal_i16) if en == 0 else en
    pa = po.calibrate(np.ascontiguousarray(signal_i16[st:en]), *calib)
    if create_events:
        cols = np.ascontiguousarray(po.detect_events(pa)[0]["mean"], np.float32) if pa.size else np.zeros(0, np.float32)
    else:
        cols = np.asarray(pa, np.float32)
    r = ac.stages(cols, kmers, mask=mask and create_events, target=target, model_target=model_target)
    r["n_events"] = cols.size
    r["dtw"] = dc.dtw(r["levels"], kmers, *dtw) if r["levels"].size else None
    return r
