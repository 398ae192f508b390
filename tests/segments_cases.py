"""TEST INFRASTRUCTURE shared by tests/test_segments_cpu.py (the kernels under the lanesim emulator) and tests/test_gpu_segments.py
(the gfx950 library): alignments in sample coordinates (unc_align_segments_batch, unc_align_ref_segments_batch).

The checker chain -- no number in it is the code under test's own:
  events     unc_o_detect_events (oracle/pyoracle.py) on the calibrated slice: mean, stdv, start, length of every kept event
  columns    align_check_mask (tests/align_check.c): which events the stall mask keeps
  path       tests/dtw_check.c on the checker's levels
  segments   tests/segments_check.c on those
Every field of every record, info and tapped event is compared in bits; results, levels and paths are compared byte for byte with
the entry point without segments, called with the same buffers full of sentinels; properties() holds for whatever comes out,
independently of the chain."""
import atexit
import ctypes as C
import shutil
import subprocess
import tempfile
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
CALIB = (1400.0, 10.0, 8192.0)          # range, offset, digitisation of the made signals
SENT8 = 0xCD
ERR_ARG = -1


# ------------------------------------------------------------------ signals (the makers of tests/golden/make_align_goldens.py)
def to_raw(pa):
    rng, off, dig = CALIB
    return np.clip(np.rint(np.asarray(pa, np.float64) * dig / rng - off), 0, 32767).astype(np.int16)


def walk_kmers(rng, n):
    bases = rng.integers(0, 4, n + 4)
    return np.array([sum(int(b) << (2 * (4 - i)) for i, b in enumerate(bases[j:j + 5])) for j in range(n)], np.uint16)


def level_signal(rng, levels, noise, dwell=(6, 14)):
    return np.concatenate([lv + noise * rng.standard_normal(int(rng.integers(*dwell))) for lv in levels])


def stall(rng, n_steps):
    """steps of 3 pA around 90 pA: events the detector sees, all within less than 5 pA"""
    return level_signal(rng, 90.0 + 1.5 * (-1.0) ** np.arange(n_steps), 0.25, dwell=(9, 12))


class Reads:
    """the made reads of the cases, one batch: 0 a walk over 300 k-mers, 1 a walk with a stall in its middle, 2 a walk whose last 40
    samples are flat (they belong to no event: the detector emits an event only at the next boundary)"""

    def __init__(self):
        from uncalled_amd import capi
        rng = np.random.default_rng(11)
        means = capi.dtw_model_tables()[0]
        self.walk = walk_kmers(rng, 300)
        lv = means[self.walk]
        self.signals = [to_raw(level_signal(rng, lv, 1.5)),
                        to_raw(np.concatenate([level_signal(rng, lv[:90], 1.5), stall(rng, 45), level_signal(rng, lv[90:180], 1.5)])),
                        to_raw(np.concatenate([level_signal(rng, lv[:60], 1.5), np.full(40, lv[60])]))]
        self.raw = np.concatenate(self.signals)
        self.offsets = np.cumsum([0] + [s.size for s in self.signals]).astype(np.uint64)
        self.calib = capi.make_calib(len(self.signals), *CALIB)


# ------------------------------------------------------------------ the checker
class SegChecker:
    _lib = None

    def __init__(self):
        if SegChecker._lib is None:
            tmp = tempfile.mkdtemp(prefix="segments_check_")
            atexit.register(shutil.rmtree, tmp, ignore_errors=True)
            so = Path(tmp) / "libsegments_check.so"
            subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", str(so), str(HERE / "segments_check.c"), "-lm"], check=True)
            L = C.CDLL(str(so))
            vp = C.c_void_p
            L.segments_check.argtypes = [vp, C.c_uint64, vp, vp, vp, vp, vp, C.c_uint64, C.c_float, C.c_float, vp, C.POINTER(C.c_uint32)]
            L.segments_check.restype = C.c_uint32
            SegChecker._lib = L

    def segments(self, path, events, col_evt, smp_st, scale, shift):
        """-> SEGMENT records, row_first"""
        from uncalled_amd import capi
        path = np.ascontiguousarray(path, np.uint32)
        f = [np.ascontiguousarray(events[k]) for k in ("mean", "stdv", "start", "length")]
        ce = np.ascontiguousarray(col_evt, np.uint32)
        out = np.zeros(int(path[:, 1].max()) + 1 if path.size else 1, capi.SEGMENT)
        rf = C.c_uint32()
        n = self._lib.segments_check(path.ctypes.data, path.shape[0], *(a.ctypes.data for a in f), ce.ctypes.data, int(smp_st),
                                     C.c_float(float(scale)), C.c_float(float(shift)), out.ctypes.data, C.byref(rf))
        return out[:n].copy(), rf.value


class Chain:
    def __init__(self, po):
        from align_check import AlignChecker
        from dtw_check import Checker
        from uncalled_amd import capi
        self.po, self.ac, self.dc, self.sc = po, AlignChecker(), Checker(), SegChecker()
        self.model_target = capi.align_model_target()

    def expected(self, signal, calib, query, kmers, opts=None, oparams=None):
        """one query through the chain -> dict(events: every kept event, col_evt, cols: the columns as events, levels, scale, shift,
        dtw: dtw_check's result or None, segs, row_first)"""
        from uncalled_amd import capi
        flags = opts.flags if opts is not None else 0
        dtw = (opts.dtw.subseq, opts.dtw.cost, opts.dtw.dw, opts.dtw.hw, opts.dtw.vw) if flags & capi.ALIGN_DTW_PARAMS else (0, 1, 1.0, 1.0, 1.0)
        st, en = query
        en = len(signal) if en == 0 else en
        pa = self.po.calibrate(np.ascontiguousarray(signal[st:en]), *calib)
        if flags & capi.ALIGN_RAW:
            ev = np.zeros(pa.size, capi.EVENT)
            ev["mean"], ev["start"], ev["length"] = pa, np.arange(pa.size), 1
        else:
            ev = self.po.detect_events(pa, oparams)[0].astype(capi.EVENT) if pa.size else np.zeros(0, capi.EVENT)
        r = self.ac.stages(ev["mean"], kmers, mask=not flags & (capi.ALIGN_RAW | capi.ALIGN_NO_MASK),
                           target="model" if flags & capi.ALIGN_TARGET_MODEL else "kmers", model_target=self.model_target)
        col_evt = np.flatnonzero(r["mask"]).astype(np.uint32)
        out = dict(events=ev, col_evt=col_evt, cols=ev[col_evt], levels=r["levels"], scale=r["scale"], shift=r["shift"], dtw=None, segs=None,
                   row_first=0)
        if r["levels"].size:
            out["dtw"] = d = self.dc.dtw(r["levels"], kmers, *dtw)
            out["segs"], out["row_first"] = self.sc.segments(d["path"], ev, col_evt, st, r["scale"], r["shift"])
        return out


# ------------------------------------------------------------------ calls through the C ABI, into buffers full of sentinels
def _sentinel(n, dt):
    return np.full(max(1, n) * np.dtype(dt).itemsize, SENT8, np.uint8).view(dt)


def call(L, reads, queries, kmers_list, opts=None, params=None, workspace=0, path_rooms="full", seg_rooms="full", evt_rooms="full",
         segments=True, refseq=None, stretches=None, want=("seg", "info", "events")):
    """unc_align_segments_batch (segments=False: unc_align_batch; with refseq and stretches the _ref_ pair) -> dict(rc, res, lev, path,
    and with segments segs, info, events: lists per query, cut to what the call says it wrote).  Asserts that every byte outside
    those counts still holds the sentinel.  rooms: "full", or a list per query"""
    from uncalled_amd import capi
    n = len(queries)
    qs = np.zeros(n, capi.ALIGN_QUERY)
    for i, (r, st, en) in enumerate(queries):
        qs[i]["read"], qs[i]["smp_st"], qs[i]["smp_en"] = r, st, en
    kms = [np.ascontiguousarray(k, np.uint16) for k in kmers_list]
    km_off = np.cumsum([0] + [k.size for k in kms]).astype(np.uint64)
    km = np.concatenate(kms + [np.zeros(1, np.uint16)])
    raw_mode = opts is not None and opts.flags & capi.ALIGN_RAW
    room = []
    for r, st, en in queries:
        ln = int(reads.offsets[r + 1] - reads.offsets[r]) if r < len(reads.offsets) - 1 else 0
        ns = max(0, (int(en) if en else ln) - int(st))
        room.append(ns if raw_mode else ns // 2 + 16)
    full_path = [c + k.size - 1 for c, k in zip(room, kms)]
    path_rooms = full_path if path_rooms == "full" else path_rooms
    seg_rooms = [k.size for k in kms] if seg_rooms == "full" else seg_rooms
    evt_rooms = room if evt_rooms == "full" else evt_rooms
    # (a query's room IS the difference of its offsets: the rooms lie one after the other, `lead` elements into the buffer)
    gap = lambda rooms, lead: (lead + np.cumsum([0] + [int(x) for x in rooms])).astype(np.uint64)     # noqa: E731
    lev_off = gap(room, 1)
    lev = _sentinel(int(lev_off[-1]) + 3, np.float32)
    res = _sentinel(n, capi.ALIGN_RESULT)
    path_off = None if path_rooms is None else gap(path_rooms, 2)
    path = None if path_rooms is None else _sentinel(2 * (int(path_off[-1]) + 3), np.uint32).reshape(-1, 2)
    head = (C.byref(params) if params is not None else None, C.byref(opts) if opts is not None else None, len(reads.offsets) - 1,
            reads.raw.ctypes.data, reads.offsets.ctypes.data, reads.calib.ctypes.data, 0, n, qs.ctypes.data)
    tail = (path.ctypes.data if path is not None else None, path_off.ctypes.data if path is not None else None)
    if refseq is not None:
        ss = capi._stretches(stretches)
        mid = (ss.ctypes.data, int(workspace), res.ctypes.data, lev.ctypes.data, lev_off.ctypes.data, None, None)
        first, old, new = refseq.h, L.unc_align_ref_batch, L.unc_align_ref_segments_batch
    else:
        mid = (km.ctypes.data, km_off.ctypes.data, int(workspace), res.ctypes.data, lev.ctypes.data, lev_off.ctypes.data)
        first, old, new = 0, L.unc_align_batch, L.unc_align_segments_batch
    out = dict(res=res, lev_buf=lev, path_buf=path, lev_off=lev_off, path_off=path_off, path_rooms=path_rooms)
    if not segments:
        out["rc"] = old(first, *head, *mid, *tail, None)
    else:
        seg_off, evt_off = gap(seg_rooms, 3), gap(evt_rooms, 1)
        seg = _sentinel(int(seg_off[-1]) + 3, capi.SEGMENT)
        info = _sentinel(n, capi.SEG_INFO)
        evt = _sentinel(int(evt_off[-1]) + 3, capi.EVENT)
        so = capi.AlignSegments()
        if "seg" in want:
            so.seg, so.seg_off = seg.ctypes.data, seg_off.ctypes.data
        if "info" in want:
            so.info = info.ctypes.data
        if "events" in want:
            so.events, so.evt_off = evt.ctypes.data, evt_off.ctypes.data
        out["rc"] = rc = new(first, *head, *mid, *tail, C.byref(so), None)
        out.update(seg_buf=seg, info=info, evt_buf=evt)
        untouched = lambda a: bool((a.view(np.uint8) == SENT8).all())       # noqa: E731
        if rc != 0:
            assert untouched(seg) and untouched(info) and untouched(evt) and untouched(res) and untouched(lev)
            assert path is None or untouched(path)
            return out
        wrote_s, wrote_e = np.zeros(seg.size, bool), np.zeros(evt.size, bool)
        out["segs"], out["events"] = [], []
        for q in range(n):
            ns = min(int(info["n_rows"][q]), int(seg_rooms[q])) if "seg" in want and "info" in want else 0
            ne = min(int(res["n_kept"][q]), int(evt_rooms[q])) if "events" in want else 0
            wrote_s[int(seg_off[q]):int(seg_off[q]) + ns] = True
            wrote_e[int(evt_off[q]):int(evt_off[q]) + ne] = True
            out["segs"].append(seg[int(seg_off[q]):int(seg_off[q]) + ns].copy())
            out["events"].append(evt[int(evt_off[q]):int(evt_off[q]) + ne].copy())
        if "info" in want or "seg" not in want:
            assert untouched(seg[~wrote_s]), "a record outside a query's room or count was written"
        assert untouched(evt[~wrote_e]), "an event outside a query's room or count was written"
        assert "info" in want or untouched(info)
    return out


def same_as_without(a, b):
    """the call with segments and the call without: return code, results, levels and paths, sentinels included"""
    assert a["rc"] == b["rc"], (a["rc"], b["rc"])
    assert a["res"].tobytes() == b["res"].tobytes(), "results differ from the call without segments"
    assert a["lev_buf"].tobytes() == b["lev_buf"].tobytes(), "levels differ from the call without segments"
    assert (a["path_buf"] is None) == (b["path_buf"] is None) and (a["path_buf"] is None or a["path_buf"].tobytes() == b["path_buf"].tobytes()), \
        "paths differ from the call without segments"


def _nan_canonical(a):
    a = a.copy()
    for f in a.dtype.names or ():
        if a.dtype[f].kind == "f":
            a[f][np.isnan(a[f])] = np.float32(np.nan)
    return a


def rec_equal(got, want):
    """every field in bits.  A NaN equals a NaN: one column against one k-mer normalises by 0 / 0 (as the reference does), and the sign
    and payload of the NaN that comes out are the processor's, not the arithmetic's"""
    return got.dtype == want.dtype and got.shape == want.shape and _nan_canonical(got).tobytes() == _nan_canonical(want).tobytes()


# ------------------------------------------------------------------ properties, whatever the chain says
def properties(segs, info, res, cols, path, query_smp_st, n_km, global_):
    """cols: the query's columns as events (the tap); path: the full path, or None"""
    from uncalled_amd import capi
    n = len(segs)
    assert n == int(info["n_rows"]) and n > 0
    assert (segs["smp_n"] <= segs["smp_span"]).all()
    assert (np.diff(segs["smp_st"].astype(np.int64)) >= 0).all()
    for s in range(n - 1):
        if segs["shared"][s + 1] == 0:
            assert int(segs["smp_st"][s + 1]) >= int(segs["smp_st"][s]) + int(segs["smp_span"][s]), s
        else:
            assert int(segs["col_first"][s + 1]) == int(segs["col_first"][s]) + int(segs["n_cols"][s]) - 1, s
    assert int(segs["shared"][0]) == 0
    if path is not None:
        assert int(segs["n_cols"].sum()) - int(segs["shared"].sum()) == np.unique(path[:, 0]).size
        assert int(info["row_first"]) == int(path[:, 1].min()) and n == np.unique(path[:, 1]).size
    if global_:
        assert int(info["row_first"]) == 0 and n == n_km
        assert int(segs["smp_st"][0]) == query_smp_st + int(cols["start"][0])
        assert int(segs["smp_st"][-1]) + int(segs["smp_span"][-1]) == query_smp_st + int(cols["start"][-1]) + int(cols["length"][-1])
    scale, shift = np.float32(res["scale"]), np.float32(res["shift"])
    with np.errstate(invalid="ignore"):      # (one column: the normaliser divides by a deviation of zero, as the reference does)
        want = (scale * segs["mean"].astype(np.float32)).astype(np.float32) + shift      # two float32 operations, each rounded
    nan = np.isnan(want)
    assert want.dtype == np.float32 and np.array_equal(nan, np.isnan(segs["level"]))
    assert np.array_equal(want.view(np.uint32)[~nan], segs["level"].view(np.uint32)[~nan])
    assert info["status"] in (capi.SEG_OK, capi.SEG_TRUNCATED)


def check_queries(chain, L, reads, queries, kmers_list, opts=None, params=None, oparams=None, workspace=0, expect_status=None, **kw):
    """the batch with and without segments (full rooms), then every query against the chain and the properties -> (call's dict,
    the chain's dicts)"""
    from uncalled_amd import capi
    a = call(L, reads, queries, kmers_list, opts, params, workspace, **kw)
    b = call(L, reads, queries, kmers_list, opts, params, workspace, segments=False, **kw)
    assert a["rc"] == 0, L.unc_last_error()
    same_as_without(a, b)
    flags = opts.flags if opts is not None else 0
    subseq = opts.dtw.subseq if flags & capi.ALIGN_DTW_PARAMS else 0
    exps = []
    for q, ((r, st, en), km) in enumerate(zip(queries, kmers_list)):
        cal = tuple(float(reads.calib[r][f]) for f in ("range", "offset", "digitisation"))
        e = chain.expected(reads.signals[r], cal, (st, en), km, opts, oparams)
        exps.append(e)
        res, info = a["res"][q], a["info"][q]
        status = int(res["status"])
        if expect_status is not None:
            assert status == expect_status[q], (q, status, expect_status[q])
        assert int(res["n_kept"]) == e["cols"].size, (q, int(res["n_kept"]), e["cols"].size)
        assert rec_equal(a["events"][q], e["cols"]), (q, "tapped events")
        if status not in (capi.DTW_OK, capi.DTW_PATH_TRUNCATED):
            assert (int(info["row_first"]), int(info["n_rows"]), int(info["status"])) == (0, 0, capi.SEG_NONE), (q, info)
            assert a["segs"][q].size == 0
            continue
        assert int(res["dtw"]["path_len"]) == e["dtw"]["path_len"], q
        assert (int(info["row_first"]), int(info["n_rows"]), int(info["status"])) == (e["row_first"], e["segs"].size, capi.SEG_OK), (q, info)
        assert rec_equal(a["segs"][q], e["segs"]), (q, a["segs"][q][:3], e["segs"][:3])
        properties(a["segs"][q], info, res, a["events"][q], e["dtw"]["path"], st, len(km), global_=subseq == 0)
    return a, exps


# ------------------------------------------------------------------ the cases: name -> function(chain, L, reads)
def _ev(dw=2.0, hw=1.0, vw=100.0, subseq=0, cost=1, **kw):
    from uncalled_amd import capi
    return capi.align_opts(dtw=capi.DTWParams(subseq, cost, dw, hw, vw), **kw)


def case_walk(chain, L, R):
    check_queries(chain, L, R, [(0, 0, 2000), (0, 500, 2500)], [R.walk[:200], R.walk[50:250]], expect_status=[0, 0])


def case_path_lengths(chain, L, R):
    """path_len of 1, 63, 64, 65, 128, 129 as one row over that many samples, and as that many rows on one sample"""
    from uncalled_amd import capi
    lens = (1, 63, 64, 65, 128, 129)
    qs = [(0, 100, 100 + n) for n in lens] + [(0, 400, 401)] * len(lens)
    kms = [R.walk[7:8]] * len(lens) + [R.walk[:n] for n in lens]
    a, _ = check_queries(chain, L, R, qs, kms, capi.align_opts(create_events=False))
    assert [int(x) for x in a["res"]["dtw"]["path_len"]] == list(lens) * 2
    assert [int(x) for x in a["info"]["n_rows"]] == [1] * len(lens) + list(lens)
    assert all(int(s["shared"][1:].min()) == 1 for s in a["segs"][len(lens) + 1:])
    # more than 128 rows on one column (case_tall's three columns guarantee more than 64 only)
    assert np.bincount(a["segs"][-1]["col_first"]).max() == 129 and int(a["segs"][-1]["shared"].sum()) == 128


def case_long_rows(chain, L, R):
    """rows of more than 64 and of more than 128 pairs"""
    from uncalled_amd import capi
    a, _ = check_queries(chain, L, R, [(0, 0, 2000), (0, 0, 900), (0, 100, 2100)], [R.walk[:2], R.walk[3:4], R.walk[9:10]],
                         capi.align_opts(mask=False))
    nc = np.concatenate([s["n_cols"] for s in a["segs"]])
    assert (nc > 128).any() and ((nc > 64) & (nc <= 128)).any(), nc


def case_tall(chain, L, R):
    """200 rows on 3 columns: more than 64 rows on one column whatever the path (more than 128 on one: case_path_lengths)"""
    from uncalled_amd import capi
    a, _ = check_queries(chain, L, R, [(0, 50, 53), (0, 300, 303)], [R.walk[:200], R.walk[100:300]], capi.align_opts(create_events=False))
    for s in a["segs"]:       # 199 moves up and 2 to the right, less what goes diagonally (at most 2)
        assert s.size == 200 and int(s["shared"].sum()) >= 197
        assert np.bincount(s["col_first"]).max() > 64


def case_stall_in_the_middle(chain, L, R):
    """the mask drops the stall's events between two kept ones.  Against the read's own 180 k-mers the rows may change right there;
    against three k-mers a row holds so many columns that one of them spans the gap"""
    a, e = check_queries(chain, L, R, [(1, 0, 0), (1, 0, 0)], [R.walk[:180], R.walk[88:91]])
    assert e[0]["col_evt"].size < e[0]["events"].size and (np.diff(e[0]["col_evt"].astype(np.int64)) > 20).any()
    assert (a["segs"][1]["smp_span"] > a["segs"][1]["smp_n"]).any()


def case_mean_limits(chain, L, R):
    """min_mean / max_mean inside the signal's range: the detector drops events within the slice"""
    from uncalled_amd import capi
    p = capi.default_params(L)
    op = chain.po.default_params()
    p.min_mean = op.min_mean = 75.0
    p.max_mean = op.max_mean = 105.0
    a, e = check_queries(chain, L, R, [(0, 0, 2500)], [R.walk[:150]], capi.align_opts(mask=False), params=p, oparams=op)
    full = chain.expected(R.signals[0], CALIB, (0, 2500), R.walk[:150], capi.align_opts(mask=False))
    assert 0 < e[0]["events"].size < full["events"].size
    assert (a["segs"][0]["smp_span"] > a["segs"][0]["smp_n"]).any()


def case_tail_without_event(chain, L, R):
    from uncalled_amd import capi
    a, e = check_queries(chain, L, R, [(2, 0, 0)], [R.walk[:60]], capi.align_opts(mask=False))
    last = a["segs"][0][-1]
    assert int(last["smp_st"]) + int(last["smp_span"]) <= R.signals[2].size - 30


def case_flags(chain, L, R):
    from uncalled_amd import capi
    check_queries(chain, L, R, [(0, 1000, 1300)], [R.walk[100:140]], capi.align_opts(create_events=False))
    check_queries(chain, L, R, [(1, 0, 0), (0, 0, 700)], [R.walk[:180], R.walk[:70]], capi.align_opts(mask=False))
    check_queries(chain, L, R, [(1, 0, 0), (0, 0, 700)], [R.walk[:180], R.walk[:70]], capi.align_opts(target="model"))


def case_subsequences(chain, L, R):
    from uncalled_amd import capi
    a, _ = check_queries(chain, L, R, [(0, 1000, 2000)], [R.walk[:300]], _ev(subseq=capi.DTW_ROW))
    assert int(a["info"]["row_first"][0]) > 0 and int(a["info"]["n_rows"][0]) < 300
    a, _ = check_queries(chain, L, R, [(0, 0, 0)], [R.walk[100:150]], _ev(subseq=capi.DTW_COL))
    assert int(a["segs"][0]["col_first"][0]) > 0 and int(a["info"]["n_rows"][0]) == 50


def case_bands(chain, L, R):
    from uncalled_amd import capi
    qs, kms = [(0, 0, 1500), (0, 200, 900)], [R.walk[:150], R.walk[20:90]]
    full, _ = check_queries(chain, L, R, qs, kms)
    for band in (150, 1 << 20):           # every cell is in the band: the full matrix's segments
        a, _ = check_queries(chain, L, R, qs, kms, capi.align_opts(band=band))
        assert all(rec_equal(x, y) for x, y in zip(a["segs"], full["segs"]))
    # 100 rows on about ten columns do not fit a band of 3; the others' rows all lie inside it
    qs, kms = [(0, 0, 900), (0, 1000, 1100), (0, 300, 1200)], [R.walk[:2], R.walk[:100], R.walk[5:8]]
    a, _ = check_queries(chain, L, R, qs, kms, capi.align_opts(band=3), expect_status=[capi.DTW_OK, capi.DTW_BAND_TOO_NARROW, capi.DTW_OK])
    assert int(a["info"]["n_rows"][1]) == 0 and int(a["info"]["n_rows"][0]) == 2 and int(a["info"]["n_rows"][2]) == 3


def case_queries_of_one_read(chain, L, R):
    a, _ = check_queries(chain, L, R, [(0, 0, 1000), (0, 700, 1900)], [R.walk[:100], R.walk[70:190]])
    assert int(a["segs"][1]["smp_st"][0]) >= 700
    a, _ = check_queries(chain, L, R, [(0, 1500, 2600), (0, 0, 1000), (0, 701, 1900)], [R.walk[150:260], R.walk[:100], R.walk[70:190]])
    assert [int(s["smp_st"][0]) >= st for s, st in zip(a["segs"], (1500, 0, 701))] == [True] * 3


def case_statuses_in_a_batch(chain, L, R):
    from uncalled_amd import capi
    o = capi.align_opts(max_events=80)       # (an event is about five samples of these reads)
    check_queries(chain, L, R, [(0, 0, 300), (0, 100, 100), (0, 0, 2000), (0, 400, 700)], [R.walk[:40], R.walk[:10], R.walk[:100], R.walk[40:80]], o,
                  expect_status=[capi.DTW_OK, capi.ALIGN_NO_COLUMNS, capi.ALIGN_TOO_MANY, capi.DTW_OK])


def case_rounds(chain, L, R):
    """back-pointers of 50 rows on about 100 columns: about 3 KB, at most two of them a round.  300 rows on 200 columns (21 KB) alone
    exceed the workspace"""
    from uncalled_amd import capi
    qs = [(0, 300 * i, 300 * i + 1000) for i in range(6)] + [(0, 0, 2000)]
    kms = [R.walk[20 * i:20 * i + 50] for i in range(6)] + [R.walk[:300]]
    one, _ = check_queries(chain, L, R, qs[:6], kms[:6])
    a, _ = check_queries(chain, L, R, qs, kms, workspace=6200, expect_status=[capi.DTW_OK] * 6 + [capi.DTW_TOO_LARGE])
    # (check_queries ends on the call without segments: the rounds of the call with them)
    call(L, R, qs, kms, workspace=6200)
    assert capi.dtw_last_timing(L)[1] >= 3
    assert all(rec_equal(x, y) for x, y in zip(a["segs"][:6], one["segs"]))
    assert int(a["info"]["n_rows"][6]) == 0 and int(a["info"]["status"][6]) == capi.SEG_NONE


def case_path_rooms(chain, L, R):
    """the caller's room for the path: none, half, all -- the same complete segments, and results and paths as without segments"""
    from uncalled_amd import capi
    qs, kms = [(0, 0, 800), (0, 900, 1500)], [R.walk[:80], R.walk[90:150]]
    full, e = check_queries(chain, L, R, qs, kms)
    lens = [int(x) for x in full["res"]["dtw"]["path_len"]]
    for rooms, st in (([0, 0], capi.DTW_PATH_TRUNCATED), ([n // 2 for n in lens], capi.DTW_PATH_TRUNCATED), (lens, capi.DTW_OK), (None, capi.DTW_OK)):
        a = call(L, R, qs, kms, path_rooms=rooms)
        b = call(L, R, qs, kms, path_rooms=rooms, segments=False)
        same_as_without(a, b)
        assert [int(s) for s in a["res"]["status"]] == [st, st]
        assert all(rec_equal(x, y["segs"]) for x, y in zip(a["segs"], e))
        assert [int(s) for s in a["info"]["status"]] == [capi.SEG_OK] * 2


def case_short_rooms(chain, L, R):
    """room for no record and for all but one: UNC_SEG_TRUNCATED, the first records, nothing outside the room (call() checks the
    sentinels); the event tap's room short in the same way; outputs left out"""
    from uncalled_amd import capi
    qs, kms = [(0, 0, 800), (0, 900, 1500)], [R.walk[:80], R.walk[90:150]]
    full, e = check_queries(chain, L, R, qs, kms)
    a = call(L, R, qs, kms, seg_rooms=[0, 59], evt_rooms=[0, e[1]["cols"].size - 1])
    assert [int(s) for s in a["info"]["status"]] == [capi.SEG_TRUNCATED] * 2 and [int(s) for s in a["info"]["n_rows"]] == [80, 60]
    assert a["segs"][0].size == 0 and rec_equal(a["segs"][1], e[1]["segs"][:59])
    assert a["events"][0].size == 0 and rec_equal(a["events"][1], e[1]["cols"][:-1])
    same_as_without(a, call(L, R, qs, kms, segments=False))
    a = call(L, R, qs, kms, want=("info",))                      # rows counted, no records asked for: none is missing
    assert [int(s) for s in a["info"]["n_rows"]] == [80, 60] and [int(s) for s in a["info"]["status"]] == [capi.SEG_OK] * 2
    big = call(L, R, qs, kms, seg_rooms=[5000, 61])              # more room than k-mers: the same records
    assert all(rec_equal(x, y["segs"]) for x, y in zip(big["segs"], e)) and [int(s) for s in big["info"]["status"]] == [capi.SEG_OK] * 2
    a = call(L, R, qs, kms, want=("events",))
    assert rec_equal(a["events"][1], e[1]["cols"])


def case_many_tiny_queries(chain, L, R):
    """more queries than the grid of k_align_segments has wavefronts (1024), and than one query per wavefront of the stages before"""
    from uncalled_amd import capi
    n = 2100
    qs = [(0, 3 * i % 2500, 3 * i % 2500 + 2 + i % 3) for i in range(n)]
    kms = [R.walk[i % 290:i % 290 + 1 + i % 4] for i in range(n)]
    a, _ = check_queries(chain, L, R, qs, kms, capi.align_opts(create_events=False))
    assert (a["info"]["status"] == capi.SEG_OK).all()


def case_argument_errors(chain, L, R):
    """UNC_ERR_ARG each, with every output untouched (call() checks the sentinels)"""
    from uncalled_amd import capi
    qs, kms = [(0, 0, 800), (0, 900, 1500)], [R.walk[:80], R.walk[90:150]]
    assert call(L, R, qs, kms, seg_rooms=[100, -50])["rc"] == ERR_ARG            # descending seg_off
    assert b"seg_off must ascend" in L.unc_last_error()
    assert call(L, R, qs, kms, evt_rooms=[500, -300])["rc"] == ERR_ARG          # descending evt_off
    assert call(L, R, [(0, 0, 800), (0, 900, R.signals[0].size + 1)], kms)["rc"] == ERR_ARG
    assert call(L, R, qs, kms, capi.align_opts(dtw=capi.DTWParams(3, 0, 1, 1, 1)))["rc"] == ERR_ARG
    # seg without seg_off, events without evt_off, no output struct: straight through the ABI
    q = np.zeros(1, capi.ALIGN_QUERY)
    q["smp_en"] = 500
    km, km_off = np.ascontiguousarray(R.walk[:50]), np.array([0, 50], np.uint64)
    res, seg, evt = _sentinel(1, capi.ALIGN_RESULT), _sentinel(60, capi.SEGMENT), _sentinel(300, capi.EVENT)
    off = np.array([0, 60], np.uint64)
    for fill in ("seg", "events", None):
        so = capi.AlignSegments()
        if fill == "seg":
            so.seg = seg.ctypes.data
        elif fill == "events":
            so.events = evt.ctypes.data
        so.info = 0
        rc = L.unc_align_segments_batch(0, None, None, len(R.offsets) - 1, R.raw.ctypes.data, R.offsets.ctypes.data, R.calib.ctypes.data, 0, 1,
                                        q.ctypes.data, km.ctypes.data, km_off.ctypes.data, 0, res.ctypes.data, None, None, None, None,
                                        C.byref(so) if fill else None, None)
        assert rc == ERR_ARG, fill
        assert all((x.view(np.uint8) == SENT8).all() for x in (res, seg, evt))
    assert off[1] == 60


CASES = {f.__name__[5:]: f for f in (case_walk, case_path_lengths, case_long_rows, case_tall, case_stall_in_the_middle, case_mean_limits,
                                     case_tail_without_event, case_flags, case_subsequences, case_bands, case_queries_of_one_read,
                                     case_statuses_in_a_batch, case_rounds, case_path_rooms, case_short_rooms, case_many_tiny_queries,
                                     case_argument_errors)}


# ------------------------------------------------------------------ the example read, by coordinates and by k-mers
def check_example(chain, G, refseq, index, prefix):
    """the example read's slice against its stretch of the reference, both strands, through unc_align_ref_segments_batch and through
    unc_align_segments_batch fed unc_ref_kmers' output: equal to each other and to the chain -> the segments"""
    from uncalled_amd import capi
    L = refseq.L
    r = len(G.signals) - 1
    qs = [(r, 10001, 14001), (r, 10001, 14001)]
    stretches = [(0, 6700, 7000, True), (0, 6700, 7000, False)]
    kms = [capi.ref_kmers(index, prefix, *s) for s in stretches]
    a, e = check_queries(chain, L, G, qs, kms)
    b = call(L, G, qs, kms, refseq=refseq, stretches=stretches)
    assert b["rc"] == 0, L.unc_last_error()
    assert all(rec_equal(x, y) for x, y in zip(a["segs"], b["segs"])) and a["info"].tobytes() == b["info"].tobytes()
    assert all(rec_equal(x, y) for x, y in zip(a["events"], b["events"])) and a["res"].tobytes() == b["res"].tobytes()
    same_as_without(b, call(L, G, qs, kms, refseq=refseq, stretches=stretches, segments=False))
    return a["segs"], kms


def check_binding_order(G, refseq, index, prefix):
    """the binding's two functions on check_example's two queries with every switch on: the length and the order of each returned
    tuple as the docstrings state them (results, levels, paths, with align_ref_batch the k-mers, then segments, their info, events),
    and every output the two routes share equal between them -- arrays byte for byte, records of floats by rec_equal"""
    from uncalled_amd import capi
    r = len(G.signals) - 1
    qs = [(r, 10001, 14001), (r, 10001, 14001)]
    stretches = [(0, 6700, 7000, True), (0, 6700, 7000, False)]
    want = [capi.ref_kmers(index, prefix, *s) for s in stretches]
    by_ref = capi.align_ref_batch(refseq, G.raw, G.offsets, G.calib, qs, stretches, levels=True, paths=True, kmers=True, segments=True, events=True)
    by_km = capi.align_batch(G.raw, G.offsets, G.calib, qs, want, levels=True, paths=True, segments=True, events=True, lib=refseq.L)
    assert isinstance(by_ref, tuple) and len(by_ref) == 7 and isinstance(by_km, tuple) and len(by_km) == 6
    res, lev, paths, kms, segs, info, evs = by_ref
    assert [k.dtype for k in kms] == [np.uint16] * 2 and [k.size for k in kms] == [296, 296]
    assert all(k.tobytes() == w.tobytes() for k, w in zip(kms, want))
    for res, lev, paths, segs, info, evs in (by_ref[:3] + by_ref[4:], by_km):      # what lies at each position
        assert isinstance(res, np.ndarray) and res.dtype == capi.ALIGN_RESULT and res.shape == (2,)
        assert [int(x) for x in res["status"]] == [capi.DTW_OK] * 2
        assert [(x.dtype, x.shape) for x in lev] == [(np.float32, (int(n),)) for n in res["n_kept"]]
        assert [(x.dtype, x.shape) for x in paths] == [(np.uint32, (int(n), 2)) for n in res["dtw"]["path_len"]]
        assert [(x.dtype, x.shape) for x in segs] == [(capi.SEGMENT, (296,))] * 2
        assert isinstance(info, np.ndarray) and info.dtype == capi.SEG_INFO and [int(x) for x in info["n_rows"]] == [296, 296]
        assert [(x.dtype, x.shape) for x in evs] == [(capi.EVENT, (int(n),)) for n in res["n_kept"]]
    a, b = by_ref[:3] + by_ref[4:], by_km
    assert a[0].tobytes() == b[0].tobytes() and a[4].tobytes() == b[4].tobytes(), "results or info differ between the routes"
    for i, name in ((1, "levels"), (2, "paths")):
        assert [x.tobytes() for x in a[i]] == [x.tobytes() for x in b[i]], name
    for i, name in ((3, "segments"), (5, "events")):
        assert all(rec_equal(x, y) for x, y in zip(a[i], b[i])), name


def check_goldens_unchanged(G, L):
    """every golden query through the new entry point with every output asked for: results, levels and paths byte for byte those
    of the old one"""
    seen = 0
    for members in G.groups():
        qs, kms = [G.query(c) for c in members], [G.kmers(c) for c in members]
        a = call(L, G, qs, kms, G.opts(members[0]))
        assert a["rc"] == 0, L.unc_last_error()
        same_as_without(a, call(L, G, qs, kms, G.opts(members[0]), segments=False))
        seen += len(members)
    return seen


def check_ref_argument_errors(G, refseq):
    """unc_align_ref_segments_batch: no output struct, seg without seg_off, events without evt_off, descending offsets, a bad stretch
    -- UNC_ERR_ARG each, every output untouched (call() checks the sentinels)"""
    from uncalled_amd import capi
    L = refseq.L
    r = len(G.signals) - 1
    qs, stretches = [(r, 10001, 11001), (r, 11001, 12001)], [(0, 6700, 6780, True), (0, 6780, 6850, False)]
    kms = [np.zeros(76, np.uint16), np.zeros(66, np.uint16)]          # (call() sizes the rooms by them)
    kw = dict(refseq=refseq, stretches=stretches)
    assert call(L, G, qs, kms, seg_rooms=[100, -50], **kw)["rc"] == ERR_ARG and b"seg_off must ascend" in L.unc_last_error()
    assert call(L, G, qs, kms, evt_rooms=[500, -300], **kw)["rc"] == ERR_ARG and b"evt_off must ascend" in L.unc_last_error()
    assert call(L, G, qs, kms, refseq=refseq, stretches=[stretches[0], (0, 6780, 6783, False)])["rc"] == ERR_ARG
    q = np.zeros(1, capi.ALIGN_QUERY)
    q["read"], q["smp_st"], q["smp_en"] = r, 10001, 11001
    ss = capi._stretches(stretches[:1])
    res, seg, evt = _sentinel(1, capi.ALIGN_RESULT), _sentinel(80, capi.SEGMENT), _sentinel(600, capi.EVENT)
    for fill in ("seg", "events", None):
        so = capi.AlignSegments()
        if fill == "seg":
            so.seg = seg.ctypes.data
        elif fill == "events":
            so.events = evt.ctypes.data
        rc = L.unc_align_ref_segments_batch(refseq.h, None, None, len(G.offsets) - 1, G.raw.ctypes.data, G.offsets.ctypes.data, G.calib.ctypes.data,
                                            0, 1, q.ctypes.data, ss.ctypes.data, 0, res.ctypes.data, None, None, None, None, None, None,
                                            C.byref(so) if fill else None, None)
        assert rc == ERR_ARG, fill
        assert all((x.view(np.uint8) == SENT8).all() for x in (res, seg, evt))
