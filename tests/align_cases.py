"""TEST INFRASTRUCTURE shared by tests/test_align_cpu.py (emulator) and tests/test_gpu_align.py (GPU): the cases of
tests/golden/align_goldens.npz as batches for capi.align_batch, and the comparison of a batch's results with them stage by stage."""
from pathlib import Path

import numpy as np

GOLD = Path(__file__).resolve().parent / "golden"
NAMES = ("tgt_mean", "tgt_stdv", "scale", "shift")


def bits(x):
    return np.asarray(x, np.float32).reshape(-1).view(np.uint32)


class Goldens:
    def __init__(self):
        from uncalled_amd import capi
        self.g = g = np.load(GOLD / "align_goldens.npz")
        ex = np.load(GOLD / "example_read.npz")
        so = g["sig_off"]
        self.signals = [g["signals"][int(so[i]):int(so[i + 1])] for i in range(so.size - 1)] + [ex["signal"]]
        self.raw = np.concatenate(self.signals).astype(np.int16)
        self.offsets = np.cumsum([0] + [s.size for s in self.signals]).astype(np.uint64)
        self.calib = capi.make_calib(len(self.signals), *map(float, g["calib"]))
        self.calib[-1] = (float(ex["range"]), float(ex["offset"]), float(ex["digitisation"]))
        self.names = [str(x) for x in g["names"]]
        self.n = len(self.names)

    def idx(self, name):
        return self.names.index(name)

    def seg(self, key, off, c):
        return self.g[key][int(self.g[off][c]):int(self.g[off][c + 1])]

    def kmers(self, c):
        return self.seg("kmers", "km_off", c)

    def query(self, c):
        return (int(self.g["sig"][c]), int(self.g["smp_st"][c]), int(self.g["smp_en"][c]))

    def opts(self, c, max_events=0):
        from uncalled_amd import capi
        o = capi.AlignOpts()
        o.flags = int(self.g["flags"][c]) | capi.ALIGN_DTW_PARAMS
        o.max_events = max_events
        o.dtw = capi.DTWParams(int(self.g["subseq"][c]), int(self.g["cost"][c]), *map(float, self.g["weights"][c]))
        return o

    def groups(self):
        """cases that share their options: one batch each"""
        out = {}
        for c in range(self.n):
            out.setdefault((int(self.g["flags"][c]), int(self.g["subseq"][c]), int(self.g["cost"][c]), tuple(map(float, self.g["weights"][c]))), []).append(c)
        return list(out.values())

    def run(self, members, lib=None, **kw):
        from uncalled_amd import capi
        return capi.align_batch(self.raw, self.offsets, self.calib, [self.query(c) for c in members], [self.kmers(c) for c in members],
                                opts=kw.pop("opts", None) or self.opts(members[0]), lib=lib, **kw)

    def check(self, c, r, lev=None, path=None):
        """one result record (and levels, path) against case c, every stage in bits"""
        from uncalled_amd import capi
        g, name = self.g, self.names[c]
        raw = bool(g["flags"][c] & capi.ALIGN_RAW)
        want_lev = self.seg("levels", "lev_off", c)
        n_in = int(self.query(c)[2] - self.query(c)[1]) if raw else self.seg("events", "ev_off", c).size
        assert int(r["n_events"]) == n_in, (name, "events detected", int(r["n_events"]), n_in)
        assert int(r["n_kept"]) == want_lev.size, (name, "events kept", int(r["n_kept"]), want_lev.size)
        for f, w in zip(NAMES[:2], g["tgt_bits"][c][:2]):
            assert int(bits(r[f])[0]) == int(w), (name, f)
        if want_lev.size == 0:
            assert int(r["status"]) == capi.ALIGN_NO_COLUMNS and int(r["dtw"]["path_len"]) == 0 and path is None, name
            return
        for f, w in zip(NAMES[2:], g["tgt_bits"][c][2:]):
            assert int(bits(r[f])[0]) == int(w), (name, f)
        if lev is not None:
            assert np.array_equal(bits(lev), bits(want_lev)), (name, "levels")
        assert int(r["status"]) == capi.DTW_OK, (name, int(r["status"]))
        assert int(bits(r["dtw"]["score"])[0]) == int(g["score_bits"][c]), (name, "score")
        assert int(bits(r["dtw"]["mean_score"])[0]) == int(g["mean_bits"][c]), (name, "mean score")
        want_path = g["path"][2 * int(g["path_off"][c]):2 * int(g["path_off"][c + 1])].reshape(-1, 2)        # (path_off counts steps, two values each)
        assert int(r["dtw"]["path_len"]) == want_path.shape[0], (name, "path length")
        if path is not None:
            assert np.array_equal(path, want_path.astype(np.uint32)), (name, "path")
