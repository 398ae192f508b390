"""TEST INFRASTRUCTURE: the banded DTW cases that tests/test_dtw_band_cpu.py (k_dtw.hip under the lanesim emulator) and
tests/test_gpu_dtw_band.py (the gfx950 library) share, and the one comparison both make: status, bits of the score, path_len, bits of
mean_score and the whole path against BandChecker.dtw (tests/dtw_band_check.c).

A batch is a dict: name, evs, kms (one array per alignment), cost, weights, band -- one call of capi.dtw_batch(..., band=W)."""
import ctypes as C

import numpy as np

import dtw_cases as dc
from dtw_band_check import LEFT_BAND, OK, TOO_NARROW, narrowest

R94P, R94D = dc.R94P, dc.R94D
SENTINEL = dc.SENTINEL
WEIGHT_SETS = [(2.0, 1.0, 100.0), (1.0, 1.0, 1.0), (0.0, 0.0, 0.0)]
ROWS = [1, 2, 63, 64, 65, 129, 200]
COLS = [1, 2, 15, 16, 17, 64, 65, 130, 300]
BANDS = [1, 2, 31, 63, 64, 65]


def band_crumb_bytes(rows, cols, band):
    """bytes of back-pointers the library holds for one banded alignment (dtw_band_crumb_words of dtw_dev.h, times 4)"""
    w = min(band, rows)
    width = min(cols, (64 + 2 * w) * cols // rows + 2)
    return 4 * 64 * ((rows + 63) // 64) * ((width + 63 + 15) // 16)


def same_float(a, b):
    """equal bits, or both NaN"""
    a, b = np.float32(a), np.float32(b)
    return (np.isnan(a) and np.isnan(b)) or dc.bits(a) == dc.bits(b)


def batch(name, evs, kms, cost, weights, band):
    assert len(evs) == len(kms)
    return dict(name=name, evs=list(evs), kms=list(kms), cost=cost, weights=tuple(weights), band=int(band))


def wanted(checker, b):
    return [checker.dtw(e, k, b["cost"], *b["weights"], b["band"]) for e, k in zip(b["evs"], b["kms"])]


def run(b, lib=None, **kw):
    from uncalled_amd import capi
    return capi.dtw_batch(b["evs"], b["kms"], capi.DTWParams(dc.NONE, b["cost"], *b["weights"]), lib=lib, full=True, band=b["band"], **kw)


def assert_equal_to_checker(res, paths, want, tag=""):
    for a, w in enumerate(want):
        at = (tag, a)
        assert int(res["status"][a]) == w["status"], (at, int(res["status"][a]), w["status"])
        assert int(res["path_len"][a]) == w["path_len"], at
        if w["status"] == TOO_NARROW:
            assert res["score"][a] == 0 and res["path_len"][a] == 0 and (paths is None or paths[a] is None), at
            continue
        assert same_float(res["score"][a], w["score"]), (at, res["score"][a], w["score"])
        assert same_float(res["mean_score"][a], w["mean"]), at
        if paths is not None:
            assert paths[a].shape == w["path"].shape and np.array_equal(paths[a], w["path"]), at


def check(checker, b, lib=None, **kw):
    """run the batch, hold every alignment against the checker -> (res, paths, want)"""
    want = wanted(checker, b)
    res, paths = run(b, lib=lib, **kw)
    assert_equal_to_checker(res, paths, want, b["name"])
    return res, paths, want


# ------------------------------------------------------------------ 2. shapes x bands
def shapes(rows=ROWS, cols=COLS):
    """every R x C of the two lists, plus R = 3 C + 1 and C = 3 R + 1"""
    out = [(r, c) for r in rows for c in cols]
    out += [(3 * c + 1, c) for c in (1, 17, 65)] + [(r, 3 * r + 1) for r in (1, 63, 65)]
    return out


def shape_batches(means, shape_list, cost, weights, seed=21):
    """One batch per W of BANDS (W >= R for the small R is among them) plus one at W = 400 >= every R, each holding every shape: the
    shapes a band cannot serve come back as too narrow beside neighbours that are computed.  Then, per shape, a batch of
    the narrowest feasible W and, where that is above 1, one of W - 1: too narrow, between two alignments that are not."""
    rng = np.random.default_rng(seed)
    kms = [rng.integers(0, 1024, r).astype(np.uint16) for r, _ in shape_list]
    evs = [dc.follow(rng, means, km, c) if n % 4 else rng.uniform(60, 130, c).astype(np.float32) for n, (km, (_, c)) in enumerate(zip(kms, shape_list))]
    out = [batch(f"shapes W {W} cost {cost} weights {weights}", evs, kms, cost, weights, W) for W in BANDS + [400]]
    by_w = {}
    for n, (r, c) in enumerate(shape_list):
        by_w.setdefault(narrowest(r, c), []).append(n)
    for W, members in sorted(by_w.items()):
        out.append(batch(f"narrowest W {W} cost {cost} weights {weights}", [evs[n] for n in members], [kms[n] for n in members], cost, weights, W))
        if W - 1 >= 1:
            small = rng.integers(0, 1024, 20).astype(np.uint16)
            pad = dc.follow(rng, means, small, 30)
            out.append(batch(f"one below the narrowest W {W} cost {cost} weights {weights}", [pad] + [evs[n] for n in members] + [pad],
                             [small] + [kms[n] for n in members] + [small], cost, weights, W - 1))
    return out


# ------------------------------------------------------------------ 3. a band that binds
def long_stay_case(means, rows=60, cols=120, stay=40, seed=22):
    """events on the k-mers' means, two per k-mer, but `stay` events in a row on one k-mer in the middle: the full matrix's path runs
    `stay` columns along one row and leaves any narrow band around the diagonal"""
    rng = np.random.default_rng(seed)
    order = rng.permutation(1024)
    km, seen = [], set()
    for k in order:         # distinct means, so that a stay costs nothing only on its own k-mer
        if float(means[k]) not in seen and len(km) < rows:
            km.append(int(k)); seen.add(float(means[k]))
    km = np.array(km, np.uint16)
    mid = rows // 2
    n_rest = cols - stay
    before = np.sort(rng.integers(0, mid, n_rest // 2))
    after = np.sort(rng.integers(mid + 1, rows, n_rest - n_rest // 2))
    idx = np.concatenate([before, np.full(stay, mid), after])
    ev = (means[km[idx]] + 0.2 * rng.standard_normal(cols)).astype(np.float32)
    return ev, km


# ------------------------------------------------------------------ 4. events that are no numbers
def nonfinite_batch(means, rows=70, cols=90, band=6, cost=R94D, weights=(1.0, 1.0, 1.0), seed=23):
    """one NaN, one +inf, one -inf event in the middle of an alignment of its own"""
    rng = np.random.default_rng(seed)
    km = rng.integers(0, 1024, rows).astype(np.uint16)
    base = dc.follow(rng, means, km, cols)
    evs = []
    for bad in (np.nan, np.inf, -np.inf):
        ev = base.copy()
        ev[cols // 2] = bad
        evs.append(ev)
    return batch("non-finite events", evs, [km] * 3, cost, weights, band)


# ------------------------------------------------------------------ 5. the C ABI as a caller may use it
def check_caller_offsets(L, checker, means, band=9, device=0, seed=24):
    """unc_dtw_band_batch with ev_off[0] = 13, km_off[0] = 7, path_off[0] = 5, NaN events and 0xFFFF k-mers outside the batch's
    stretch, rooms for the paths of: the length + 3, the length, 5 short, 0, 1; sentinels around and between."""
    from uncalled_amd import capi
    rng = np.random.default_rng(seed)
    shape_list = [(70, 50), (33, 130), (64, 64), (20, 90), (90, 15)]
    cost, weights = R94P, (2.0, 1.0, 100.0)
    kms = [rng.integers(0, 1024, r).astype(np.uint16) for r, _ in shape_list]
    evs = [dc.follow(rng, means, km, c) for km, (_, c) in zip(kms, shape_list)]
    want = [checker.dtw(e, k, cost, *weights, band) for e, k in zip(evs, kms)]
    assert all(w["status"] == OK for w in want)
    need = [w["path_len"] for w in want]
    rooms = [need[0] + 3, need[1], need[2] - 5, 0, 1]
    ev = np.concatenate([np.full(13, np.nan, np.float32)] + evs + [np.full(9, np.nan, np.float32)])
    km = np.concatenate([np.full(7, 0xFFFF, np.uint16)] + kms + [np.full(9, 0xFFFF, np.uint16)])
    ev_off = (13 + np.cumsum([0] + [e.size for e in evs])).astype(np.uint64)
    km_off = (7 + np.cumsum([0] + [k.size for k in kms])).astype(np.uint64)
    path_off = (5 + np.cumsum([0] + rooms)).astype(np.uint64)
    path = np.full((int(path_off[-1]) + 64, 2), SENTINEL, np.uint32)
    res = np.zeros(len(shape_list), capi.DTW_RESULT)
    prm = capi.DTWParams(dc.NONE, cost, *weights)
    rc = L.unc_dtw_band_batch(device, len(shape_list), ev.ctypes.data, ev_off.ctypes.data, km.ctypes.data, km_off.ctypes.data, C.byref(prm), band,
                              0, res.ctypes.data, path.ctypes.data, path_off.ctypes.data, None)
    assert rc == 0
    written = np.zeros(path.shape[0], bool)
    for a, w in enumerate(want):
        got = min(need[a], rooms[a])
        assert res["status"][a] == (capi.DTW_OK if rooms[a] >= need[a] else capi.DTW_PATH_TRUNCATED), a
        assert dc.bits(res["score"][a]) == w["score_bits"] and dc.bits(res["mean_score"][a]) == dc.bits(w["mean"]), a
        assert int(res["path_len"][a]) == need[a], a
        at = int(path_off[a])
        assert np.array_equal(path[at:at + got], w["path"][:got]), a
        written[at:at + got] = True
    assert (path[~written] == SENTINEL).all()
    # no alignments: accepted, nothing to do, and the timing says so
    ms, rounds, held = C.c_float(1), C.c_uint32(1), C.c_uint64(1)
    rc = L.unc_dtw_band_batch(device, 0, ev.ctypes.data, ev_off.ctypes.data, km.ctypes.data, km_off.ctypes.data, C.byref(prm), band, 0,
                              res.ctypes.data, None, None, None)
    assert rc == 0
    L.unc_dtw_last_timing(C.byref(ms), C.byref(rounds), C.byref(held))
    assert (ms.value, rounds.value, held.value) == (0.0, 0, 0)


def check_argument_errors(lib):
    from uncalled_amd import capi
    ev, km = np.full(4, 90, np.float32), np.arange(4, dtype=np.uint16)
    res = np.zeros(1, capi.DTW_RESULT)
    off = np.array([0, 4], np.uint64)
    for subseq, band in ((dc.NONE, 0), (dc.ROW, 3), (dc.COL, 3)):
        prm = capi.DTWParams(subseq, R94D, 1, 1, 1)
        rc = lib.unc_dtw_band_batch(0, 1, ev.ctypes.data, off.ctypes.data, km.ctypes.data, off.ctypes.data, C.byref(prm), band, 0, res.ctypes.data,
                                    None, None, None)
        assert rc == -1, (subseq, band, rc)         # UNC_ERR_ARG
    # what unc_dtw_batch refuses is refused here too
    import pytest
    for evs, kms, prm in (([ev[:0]], [km], capi.DTWParams(0, 0, 1, 1, 1)), ([ev], [km + 1021], capi.DTWParams(0, 0, 1, 1, 1)),
                          ([ev], [km], capi.DTWParams(3, 0, 1, 1, 1)), ([ev], [km], capi.DTWParams(0, 2, 1, 1, 1))):
        with pytest.raises(capi.UncalledHipError, match="error -1"):
            capi.dtw_batch(evs, kms, prm, lib=lib, band=3)


def rounds_batch(means, n=12, seed=25):
    """12 alignments of about 100 x 150 at W = 8 and a workspace that holds four of them"""
    rng = np.random.default_rng(seed)
    shape_list = [(100 + 3 * a, 150 - 2 * a) for a in range(n)]
    kms = [rng.integers(0, 1024, r).astype(np.uint16) for r, _ in shape_list]
    evs = [dc.follow(rng, means, km, c) for km, (_, c) in zip(kms, shape_list)]
    b = batch("rounds", evs, kms, R94D, (1.0, 1.0, 1.0), 8)
    sizes = [band_crumb_bytes(r, c, 8) for r, c in shape_list]
    b["workspace"] = sum(sorted(sizes)[-4:])
    b["sizes"] = sizes
    return b


def check_rounds_and_too_large(checker, means, lib=None):
    from uncalled_amd import capi
    b = rounds_batch(means)
    res0, paths0, want = check(checker, b, lib=lib)
    assert capi.dtw_last_timing(lib)[1] == 1
    res1, paths1 = run(b, lib=lib, workspace_bytes=b["workspace"])
    ms, rounds, held = capi.dtw_last_timing(lib)
    assert rounds >= 3 and held <= b["workspace"], (rounds, held)
    assert_equal_to_checker(res1, paths1, want, "rounds")
    # one alignment too large for the workspace: reported, the others computed
    sizes = b["sizes"] + [band_crumb_bytes(400, 400, 8)]
    rng = np.random.default_rng(26)
    km = rng.integers(0, 1024, 400).astype(np.uint16)
    big = batch("too large", b["evs"] + [dc.follow(rng, means, km, 400)], b["kms"] + [km], b["cost"], b["weights"], 8)
    assert sizes[-1] > max(sizes[:-1])
    res, paths = run(big, lib=lib, workspace_bytes=sizes[-1] - 1)
    assert res["status"][-1] == capi.DTW_TOO_LARGE and res["path_len"][-1] == 0 and res["score"][-1] == 0 and paths[-1] is None
    assert_equal_to_checker(res[:-1], paths[:-1], want, "too large")


# ------------------------------------------------------------------ 6. the align pipeline
def check_align(G, lib, checker, narrow=4):
    """align_batch with opts.band on the global-alignment cases of tests/align_cases.py: the band checker on the tapped levels and
    the k-mers must give status, score, mean and path, for a narrow band (it binds: some query's score differs from the full matrix's)
    and for W >= R (everything equals the full matrix's); band = 0 is today's call.  -> queries compared"""
    from uncalled_amd import capi
    binds = compared = 0
    for members in G.groups():
        c0 = members[0]
        if int(G.g["subseq"][c0]) != dc.NONE:
            continue
        cost, weights = int(G.g["cost"][c0]), tuple(map(float, G.g["weights"][c0]))
        full, lev_f, path_f = G.run(members, lib=lib, levels=True, paths=True)
        o = G.opts(c0)
        o.band = 0
        zero, _, path_z = G.run(members, lib=lib, levels=True, paths=True, opts=o)
        assert full.tobytes() == zero.tobytes()
        assert all((a is None and b is None) or np.array_equal(a, b) for a, b in zip(path_f, path_z))
        for W in (narrow, 1 << 20):
            o = G.opts(c0)
            o.band = W
            res, levs, paths = G.run(members, lib=lib, levels=True, paths=True, opts=o)
            for q, c in enumerate(members):
                assert np.array_equal(dc_bits_all(levs[q]), dc_bits_all(lev_f[q])), (W, c)
                if int(full["status"][q]) == capi.ALIGN_NO_COLUMNS:
                    assert res[q].tobytes() == full[q].tobytes() and paths[q] is None
                    continue
                w = checker.dtw(levs[q], G.kmers(c), cost, *weights, W)
                assert int(res["status"][q]) == w["status"], (W, c)
                assert int(res["dtw"]["path_len"][q]) == w["path_len"], (W, c)
                compared += 1
                if w["status"] == TOO_NARROW:
                    assert res["dtw"]["score"][q] == 0 and paths[q] is None, (W, c)
                    continue
                assert same_float(res["dtw"]["score"][q], w["score"]) and same_float(res["dtw"]["mean_score"][q], w["mean"]), (W, c)
                assert np.array_equal(paths[q], w["path"]), (W, c)
                if W == narrow:
                    binds += dc.bits(res["dtw"]["score"][q]) != dc.bits(full["dtw"]["score"][q])
                else:
                    assert res[q].tobytes() == full[q].tobytes() and np.array_equal(paths[q], path_f[q]), c
    assert binds >= 1 and compared >= 4, (binds, compared)
    return compared


def dc_bits_all(x):
    return np.asarray(x, np.float32).reshape(-1).view(np.uint32)
