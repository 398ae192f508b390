"""TEST INFRASTRUCTURE: the adaptive band with an open end (UNC_ALIGN_ADAPTIVE) through the features it is shipped with -- a custom
pore model, the training accumulator, the pile-up, the rounds, the other options of the align pipeline -- shared by
tests/test_dtw_adapt_cpu.py (the align emulator library) and tests/test_gpu_dtw_adapt.py (the gfx950 library).

Every comparison is in bits or integers against a checker the project trusts already: AdaptChecker (tests/dtw_adapt_check.c) on the
returned levels and k-mers with the tables of the model in use, SegChecker (tests/segments_check.c) on that path and the returned
events, model_naive and pileup_naive on the returned records.  P is the context: the library, the example read and index, a random
model and the checkers, made once a module."""
import ctypes as C

import numpy as np

import align_cases as ac
import dtw_adapt_cases as xc
import model_cases as mc
import model_naive as mn
import pileup_cases as pc
import segments_cases as sc
from dtw_adapt_check import LEFT_BAND, OK, REF_END, AdaptChecker, adapt_crumb_bytes

BAND = 128


class Ctx:
    def __init__(self, L, prefix):
        from uncalled_amd import capi
        self.L = L
        self.G = ac.Goldens()
        self.X = pc.Ctx(L, prefix)
        self.model = capi.Model.from_pairs(mc.random_pairs(15), lib=L)         # (case_random_model_alignment's)
        self.default_checker = AdaptChecker()
        self.model_checker = AdaptChecker(model=self.model.tables(False)[:3])
        self.segck = sc.SegChecker()
        r = len(self.G.signals) - 1
        # the example read's slice against both example stretches, and four more slices of it: six queries
        self.qs = [(r, 10001, 14001), (r, 10001, 14001), (r, 10401, 14001), (r, 10001, 13001), (r, 11001, 14001), (r, 10201, 13801)]
        self.stretches = [xc.EXAMPLE_STRETCHES[q % 2] for q in range(len(self.qs))]
        self._base = {}

    def run(self, opts=None, qs=None, stretches=None, **kw):
        """-> (res, levels, paths, kmers, segments, info, events)"""
        from uncalled_amd import capi
        opts = capi.align_opts(adaptive=BAND) if opts is None else opts
        return capi.align_ref_batch(self.X.refseq, self.G.raw, self.G.offsets, self.G.calib, self.qs if qs is None else qs,
                                    self.stretches if stretches is None else stretches, opts, levels=True, paths=True, kmers=True,
                                    segments=True, events=True, **kw)

    def trained(self, keep):
        """the six queries with the random model, an accumulator and a pile-up, in one round -> (out, acc, pileup)"""
        from uncalled_amd import capi
        if keep not in self._base:
            acc, pu = capi.ModelAcc(keep_shared=keep, lib=self.L), self.X.pileup(None, keep)
            self._base[keep] = (self.run(model=self.model, accumulate=acc, pileup=pu), acc, pu)
            assert capi.dtw_last_timing(self.L)[1] == 1
        return self._base[keep]


def hold(P, out, checker, band=BAND, only=None, qs=None):
    """status, bits of the score and of the mean score, path_len and path against the checker on the returned levels and k-mers; the
    segments against SegChecker on the checker's path and the returned events -> the checker's results"""
    from uncalled_amd import capi
    res, levs, paths, kms, segs, info, events = out
    qs = P.qs if qs is None else qs
    wants = []
    for q in range(len(res)) if only is None else only:
        w = checker.dtw(levs[q], kms[q], xc.R94D, 1.0, 1.0, 1.0, band)
        wants.append(w)
        assert w["status"] in (OK, REF_END) and int(res["status"][q]) == w["status"], (q, int(res["status"][q]), w["status"])
        assert xc.same_float(res["dtw"]["score"][q], w["score"]) and xc.same_float(res["dtw"]["mean_score"][q], w["mean"]), q
        assert int(res["dtw"]["path_len"][q]) == w["path_len"] and np.array_equal(paths[q], w["path"]), q
        want_seg, row_first = P.segck.segments(w["path"], events[q], np.arange(events[q].size, dtype=np.uint32), qs[q][1], res["scale"][q],
                                               res["shift"][q])
        assert (int(info["status"][q]), int(info["row_first"][q]), int(info["n_rows"][q])) == (capi.SEG_OK, row_first, want_seg.size), (q, info[q])
        assert row_first == 0 and want_seg.size == w["end_row"] + 1 and sc.rec_equal(segs[q], want_seg), q
    return wants


def same_outputs(a, b, only=None):
    """results, levels, paths, k-mers, segments, info and events of two calls, byte for byte"""
    idx = range(len(a[0])) if only is None else only
    for q in idx:
        assert a[0][q].tobytes() == b[0][q].tobytes(), (q, a[0][q], b[0][q])
        for i in (1, 2, 3, 6):
            assert (a[i][q] is None and b[i][q] is None) or a[i][q].tobytes() == b[i][q].tobytes(), (q, i)
        assert sc.rec_equal(a[4][q], b[4][q]) and a[5][q].tobytes() == b[5][q].tobytes(), q


# ------------------------------------------------------------------ 1. a custom model
def check_custom_model(P):
    """the rows' model values are read from the table of the model in use, at the band's first fill and 64 at a time as it moves down"""
    out = P.run(model=P.model)
    wants = hold(P, out, P.model_checker)
    assert any(w["lo"].max() >= 64 - BAND // 2 for w in wants)          # the band moved down past one reload of 64 rows
    base = P.run()
    hold(P, base, P.default_checker)
    assert out[0]["dtw"].tobytes() != base[0]["dtw"].tobytes() and any(not np.array_equal(a, b) for a, b in zip(out[2], base[2]))


# ------------------------------------------------------------------ 2. training with an open end
def check_training(P, keep):
    """the accumulator holds exactly the returned records over the k-mers [row_first, row_first + n_rows): an open end stops at row
    n_rows - 1 < rows - 1, and the k-mers behind it add nothing"""
    out, acc, pu = P.trained(keep)
    res, levs, paths, kms, segs, info, events = out
    hold(P, out, P.model_checker)
    want = mc.naive_of_segments(kms, segs, info, keep)
    got = mc.read_equals(acc, want)
    open_end = [q for q in range(len(res)) if int(res["status"][q]) == OK and int(info["n_rows"][q]) < kms[q].size]
    assert open_end and sum(want["n"]) > 300
    on_paths = set()
    for q in range(len(res)):
        on_paths |= set(int(k) for k in kms[q][int(info["row_first"][q]):int(info["row_first"][q]) + int(info["n_rows"][q])])
    behind = set(int(k) for q in open_end for k in kms[q][int(info["n_rows"][q]):]) - on_paths
    assert len(behind) > 20 and all(got["n"][k] == 0 and got["S"][k] == 0 and got["SS"][k] == 0 for k in behind)
    m, kept = acc.finish(P.model, 2)
    want_pairs, want_kept = mn.finish(want, P.model.pairs(), 2)
    assert m.pairs().tobytes() == want_pairs.tobytes() and kept == want_kept
    assert m.pairs().tobytes() != P.model.pairs().tobytes()
    # the pile-up of the same call: the naive pile-up of the same records
    nv = pc.naive_of_segments(pc.whole(P.X), P.stretches, segs, info, keep)
    assert nv.added > 300
    pc.equals_naive(pu, nv)


# ------------------------------------------------------------------ 3. rounds through the hook
def check_rounds(P, keep=False):
    """a workspace that holds two of the six alignments: results, paths, segments, accumulator and pile-up equal the one-round run"""
    from uncalled_amd import capi
    one, acc1, pu1 = P.trained(keep)
    sizes = sorted(adapt_crumb_bytes(k.size, int(c), BAND) for k, c in zip(one[3], one[0]["n_kept"]))
    acc, pu = capi.ModelAcc(keep_shared=keep, lib=P.L), P.X.pileup(None, keep)
    out = P.run(model=P.model, accumulate=acc, pileup=pu, workspace_bytes=sizes[-1] + sizes[-2])
    rounds, held = capi.dtw_last_timing(P.L)[1:]
    assert rounds >= 3 and held <= sizes[-1] + sizes[-2], (rounds, held, sizes)
    same_outputs(out, one)
    assert mn.of_read(acc.read()) == mn.of_read(acc1.read())
    assert pc.table(pu).tobytes() == pc.table(pu1).tobytes() and pu.counters() == pu1.counters()


# ------------------------------------------------------------------ 4. the other options
def check_options(P):
    from uncalled_amd import capi
    base = P.run()
    hold(P, base, P.default_checker)
    tm = P.run(capi.align_opts(adaptive=BAND, target="model"))
    hold(P, tm, P.default_checker)
    assert tm[0]["scale"].tobytes() != base[0]["scale"].tobytes()
    nm = P.run(capi.align_opts(adaptive=BAND, mask=False))
    hold(P, nm, P.default_checker)
    assert (nm[0]["n_kept"] == nm[0]["n_events"]).all() and (nm[0]["n_kept"] >= base[0]["n_kept"]).all()
    # max_events one below the most columns a query has: that query (and its twin on the other strand) is not aligned
    kept = [int(x) for x in base[0]["n_kept"]]
    limit = max(kept) - 1
    many = [q for q, n in enumerate(kept) if n > limit]
    rest = [q for q, n in enumerate(kept) if n <= limit]
    assert many and len(rest) >= 3
    acc = capi.ModelAcc(lib=P.L)
    cut = P.run(capi.align_opts(adaptive=BAND, max_events=limit), accumulate=acc)
    for q in many:
        assert int(cut[0]["status"][q]) == capi.ALIGN_TOO_MANY and cut[2][q] is None and int(cut[0]["dtw"]["path_len"][q]) == 0
        assert (int(cut[5]["status"][q]), int(cut[5]["n_rows"][q])) == (capi.SEG_NONE, 0)
    same_outputs(cut, base, only=rest)
    hold(P, cut, P.default_checker, only=rest)
    mc.read_equals(acc, mc.naive_of_segments([cut[3][q] for q in rest], [cut[4][q] for q in rest], cut[5][rest]))
    # a caller's room for segments five records short of n_rows
    G = P.G
    n_rows = [int(x) for x in base[5]["n_rows"]]
    assert min(n_rows) > 5
    a = sc.call(P.L, G, P.qs, base[3], capi.align_opts(adaptive=BAND), seg_rooms=[n - 5 for n in n_rows], refseq=P.X.refseq, stretches=P.stretches)
    assert a["rc"] == 0 and (a["info"]["status"] == capi.SEG_TRUNCATED).all()
    assert [int(x) for x in a["info"]["n_rows"]] == n_rows and a["res"].tobytes() == base[0].tobytes()
    for q, w in enumerate(hold(P, base, P.default_checker)):
        want_seg, _ = P.segck.segments(w["path"], base[6][q], np.arange(base[6][q].size, dtype=np.uint32), P.qs[q][1], base[0]["scale"][q],
                                       base[0]["shift"][q])
        assert a["segs"][q].size == n_rows[q] - 5 and sc.rec_equal(a["segs"][q], want_seg[:n_rows[q] - 5]), q
    # (sc.call has asserted that every record behind the rooms still holds the sentinel)


# ------------------------------------------------------------------ 5. a path without a start
def check_left_band(P, band=64):
    """UNC_ALIGN_RAW and a read whose calibration has digitisation 0: every sample of that read is not a number, and so is every
    level and every score.  No score compares, so the band moves by parity alone, the end cell is the last column's last computed
    cell and every back-pointer says V: with more rows than the band holds, the traceback climbs the last column out of the band.
    The query has UNC_DTW_LEFT_BAND and the pairs so far, no segments (UNC_SEG_NONE), and adds nothing to the accumulator or the
    pile-up; the healthy queries beside it are those of the batch without it."""
    from uncalled_amd import capi
    R = sc.Reads()
    calib = R.calib.copy()
    calib[1] = (1400.0, 10.0, 0.0)
    qs = [(0, 300, 450), (1, 100, 250), (2, 0, 150)]
    stretches = [(0, 100, 254, True), (0, 300, 454, False), (0, 5000, 5154, True)]
    o = capi.align_opts(create_events=False, adaptive=band)
    kw = dict(levels=True, paths=True, kmers=True, segments=True, events=True)
    healthy = [0, 2]

    def call(which, **more):
        return capi.align_ref_batch(P.X.refseq, R.raw, R.offsets, calib, [qs[q] for q in which], [stretches[q] for q in which], o, **kw, **more)

    for keep in (False, True):
        acc, pu = capi.ModelAcc(keep_shared=keep, lib=P.L), P.X.pileup(None, keep)
        res, levs, paths, kms, segs, info, events = out = call([0, 1, 2], accumulate=acc, pileup=pu)
        assert not np.isfinite(levs[1]).any() and kms[1].size == 150 > band
        w = P.default_checker.dtw(levs[1], kms[1], xc.R94D, 1.0, 1.0, 1.0, band)
        assert w["status"] == LEFT_BAND and 0 < w["path_len"] < 150
        assert int(res["status"][1]) == LEFT_BAND and int(res["dtw"]["path_len"][1]) == w["path_len"] and np.array_equal(paths[1], w["path"])
        assert int(w["path"][-1][1]) > 0 and int(w["path"][-1][0]) == 149          # the path's last pair is no start: row_first would be wrong
        assert (int(info["status"][1]), int(info["row_first"][1]), int(info["n_rows"][1])) == (capi.SEG_NONE, 0, 0) and segs[1].size == 0
        acc2, pu2 = capi.ModelAcc(keep_shared=keep, lib=P.L), P.X.pileup(None, keep)
        alone = call(healthy, accumulate=acc2, pileup=pu2)
        for i, q in enumerate(healthy):
            assert int(res["status"][q]) in (OK, REF_END) and int(info["status"][q]) == capi.SEG_OK
            for f in (0, 1, 2, 3, 5, 6):
                assert out[f][q].tobytes() == alone[f][i].tobytes(), (q, f)
            assert sc.rec_equal(segs[q], alone[4][i])
            wq = P.default_checker.dtw(levs[q], kms[q], xc.R94D, 1.0, 1.0, 1.0, band)
            assert int(res["status"][q]) == wq["status"] and np.array_equal(paths[q], wq["path"]) and xc.same_float(res["dtw"]["score"][q], wq["score"])
        want = mc.naive_of_segments([kms[q] for q in healthy], [segs[q] for q in healthy], info[healthy], keep)
        assert sum(want["n"]) > 20
        mc.read_equals(acc, want)
        nv = pc.naive_of_segments(pc.whole(P.X), [stretches[q] for q in healthy], [segs[q] for q in healthy], info[healthy], keep)
        assert nv.added > 20
        pc.equals_naive(pu, nv)
