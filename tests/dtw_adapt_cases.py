"""TEST INFRASTRUCTURE: the adaptive-band DTW cases that tests/test_dtw_adapt_cpu.py (k_dtw_adapt.hip under the lanesim emulator) and
tests/test_gpu_dtw_adapt.py (the gfx950 library) share, and the one comparison both make: status, bits of the score, path_len, bits
of mean_score and the whole path against AdaptChecker.dtw (tests/dtw_adapt_check.c).

A batch is a dict: name, evs, kms (one array per alignment), cost, weights, band -- one call of capi.dtw_batch(..., adaptive=B)."""
import ctypes as C

import numpy as np

import dtw_cases as dc
from dtw_adapt_check import LEFT_BAND, OK, REF_END, adapt_crumb_bytes
from dtw_band_cases import same_float

R94P, R94D = dc.R94P, dc.R94D
SENTINEL = dc.SENTINEL
WEIGHT_SETS = [(2.0, 1.0, 100.0), (1.0, 1.0, 1.0)]


def batch(name, evs, kms, cost, weights, band):
    assert len(evs) == len(kms)
    return dict(name=name, evs=list(evs), kms=list(kms), cost=cost, weights=tuple(weights), band=int(band))


def wanted(checker, b):
    return [checker.dtw(e, k, b["cost"], *b["weights"], b["band"]) for e, k in zip(b["evs"], b["kms"])]


def run(b, lib=None, **kw):
    from uncalled_amd import capi
    return capi.dtw_batch(b["evs"], b["kms"], capi.DTWParams(dc.NONE, b["cost"], *b["weights"]), lib=lib, full=True, adaptive=b["band"], **kw)


def assert_equal_to_checker(res, paths, want, tag=""):
    for a, w in enumerate(want):
        at = (tag, a)
        assert int(res["status"][a]) == w["status"], (at, int(res["status"][a]), w["status"])
        assert int(res["path_len"][a]) == w["path_len"], at
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


# ------------------------------------------------------------------ 1. shapes
SHAPES_64 = [(1, 1), (1, 40), (40, 1), (5, 5), (70, 70), (200, 300), (1, 63), (1, 64), (1, 65)]      # rows, cols


def case_of_path_len(checker, means, want_len, cost, weights, band=64):
    """the first of a seeded run of follow cases -- 90 k-mers at B = 64, 1.5 B at the wider bands, so that the band has rows to move
    to -- against `want_len` events and fewer (a path has one pair an event and one more for every V move), whose path, by the
    checker, has exactly `want_len` pairs"""
    rows = 90 if band == 64 else band + band // 2
    for cols in range(want_len, want_len - 40, -1):
        for seed in range(10):
            ev, km = follow_case(np.random.default_rng(1000 + seed), means, rows, cols)
            if checker.dtw(ev, km, cost, *weights, band)["path_len"] == want_len:
                return ev, km
    raise AssertionError("no case with a path of %d pairs" % want_len)


def follow_case(rng, means, rows, cols, used=None, noise=1.5):
    """events that follow the first `used` of `rows` k-mers (default: two thirds of them: the stretch is 1.5 times too long)"""
    km = rng.integers(0, 1024, rows).astype(np.uint16)
    used = max(1, (2 * rows) // 3) if used is None else used
    return dc.follow(rng, means, km[:used], cols, noise), km


def shape_batches(means, cost, weights, seed=41):
    """B = 64: shapes smaller than the band, 70 x 70 and 200 x 300 (the band leaves row 0 and crosses several words of back-pointers),
    one k-mer against 63, 64 and 65 events (paths of exactly so many pairs, around the flush of 64; case_of_path_len gives 128), k-mers that run out (the events follow all of them: UNC_DTW_REF_END) and three times too many k-mers.  B = 128 and 256: 300 x 400, two and four cells a lane."""
    rng = np.random.default_rng(seed)
    evs, kms = zip(*([follow_case(rng, means, r, c) for r, c in SHAPES_64]))
    short = [follow_case(rng, means, 60, 200, used=60), follow_case(rng, means, 100, 130, used=100)]
    long_ = [follow_case(rng, means, 300, 150, used=100)]
    out = [batch(f"shapes B 64 cost {cost} weights {weights}", evs, kms, cost, weights, 64),
           batch(f"k-mers run out, B 64 cost {cost} weights {weights}", [e for e, _ in short + long_], [k for _, k in short + long_], cost, weights, 64)]
    for B in (128, 256):
        ev, km = follow_case(rng, means, 300, 400)
        out.append(batch(f"300 x 400 B {B} cost {cost} weights {weights}", [ev], [km], cost, weights, B))
    return out


# ------------------------------------------------------------------ 1b. the band's width edges, at every width
EDGE_COLS = (1, 2, 63, 64, 65, 129)


def edge_rows(B):
    """around B / 2 (the initial fill ends; the band holds the last row from the start), around B (the first move down loads the
    model's block at B / 2; the band comes to hold the last row after a few moves), and above"""
    return (B // 2 - 1, B // 2, B // 2 + 1, B - 1, B, B + 1, B + B // 2 + 1)


def edge_batches(means, cost, weights, B, seed=64):
    """two batches of the 7 x 6 = 42 shapes edge_rows(B) x EDGE_COLS: the events follow the first two thirds of the k-mers (the end
    is open), and all of them (the k-mers run out)"""
    shapes = [(r, c) for r in edge_rows(B) for c in EDGE_COLS]
    out = []
    for name, all_rows in (("two thirds", False), ("all", True)):
        rng = np.random.default_rng(seed)
        evs, kms = zip(*[follow_case(rng, means, r, c, used=r if all_rows else None) for r, c in shapes])
        out.append(batch(f"edges B {B}, events follow {name} of the k-mers, cost {cost} weights {weights}", evs, kms, cost, weights, B))
    return out


def check_edges(checker, means, B, lib=None):
    """edge_batches at width B under both costs and both weight sets against the checker, and, by the checker alone, what the
    alignments are there to reach (over the four combinations together: with dw = 2 hw the band of these shapes hardly moves)"""
    flat = []
    for cost in (R94P, R94D):
        for weights in WEIGHT_SETS:
            for b in edge_batches(means, cost, weights, B):
                assert len(b["evs"]) == 42 and max(k.size for k in b["kms"]) == B + B // 2 + 1
                _, _, want = check(checker, b, lib=lib)
                flat += [(k.size, w) for k, w in zip(b["kms"], want)]
    assert {w["status"] for _, w in flat} == {OK, REF_END}
    assert any(w["lo"].max() > 0 for _, w in flat)                                     # a band that left row 0
    assert any((w["lo"] == -B // 2).all() for _, w in flat)                            # a band that never moved
    # rows > B: the band does not hold the last row at first and comes to hold it: the clamp switches on in mid-sweep
    assert any(rows > B and w["lo"][0] + B - 1 < rows - 1 and w["lo"][-1] + B - 1 == rows - 1 for rows, w in flat)


def n_done_case(checker, ev, km, B, cost, weights):
    """-> the checker's result if the sweep ended early (an anti-diagonal without a present cell) and an end cell exists, else None"""
    w = checker.dtw(ev, km, cost, *weights, B)
    if w["lo"].size < ev.size + km.size - 1 and w["end_row"] is not None:
        return w
    return None


def early_end_family(means, B):
    """3 B k-mers against 140 events and fewer that follow the first 8 to 23 of them, then the first B / 4 and more: the last column
    passes below the band"""
    for cols in range(140, 76, -1):
        for used in (8, 11, 14, 17, 20, 23) + tuple(range(B // 4, B, 4)):
            yield follow_case(np.random.default_rng(2000 + used), means, 3 * B, cols, used=used)


def case_of_n_done(checker, means, B, residue64, cost, weights, end_in_last_block=False):
    """-> (ev, km, the checker's result) of the first case of early_end_family whose sweep ends early, at n_done < rows + cols - 1
    anti-diagonals, with n_done % 64 == residue64 and, if asked for, the end cell's anti-diagonal in the last block of 64.  (An early
    end comes after an ODD number of anti-diagonals -- tests/test_dtw_adapt_cpu.py states why -- so for an even residue this raises.)"""
    for ev, km in early_end_family(means, B):
        w = n_done_case(checker, ev, km, B, cost, weights)
        if w is not None and w["lo"].size % 64 == residue64 and (not end_in_last_block or end_in_last_partial_block(w, ev.size)):
            return ev, km, w
    raise AssertionError("no case whose sweep ends early after a number of anti-diagonals that is %d modulo 64" % residue64)


def full_sweep_case(means, B, residue64, seed=48):
    """B / 2 k-mers (the band holds the last row from the start: the sweep runs to its end) against as many events, 65 or more, as
    make rows + cols - 1 == residue64 modulo 64"""
    rows = B // 2
    cols = 65 + (residue64 - rows - 64) % 64
    assert (rows + cols - 1) % 64 == residue64
    return follow_case(np.random.default_rng(seed), means, rows, cols)


N_DONE_RESIDUES = (0, 1, 15, 16, 17, 63)
N_DONE_TIE_COLS = (65, 66, 73)


def n_done_tie_case(means, B, cols):
    """all-equal events, weights 0: every move is a tie, lo_d = -B / 2 + d // 2, and with 3 B rows the last column's row d - (cols - 1)
    passes lo_d + B - 1 at d = B + 2 cols - 3: that many anti-diagonals are computed (63, 1 and 15 modulo 64 for 65, 66, 73 events)"""
    return np.full(cols, means[77], np.float32), np.full(3 * B, 77, np.uint16), B + 2 * cols - 3


def end_in_last_partial_block(w, cols):
    """the end cell's anti-diagonal lies in the last block of 64 lo_d, and that block is not full"""
    n_done = w["lo"].size
    return n_done % 64 != 0 and (w["end_row"] + cols - 1) // 64 == (n_done - 1) // 64


def check_early_end(checker, means, B, lib=None):
    """n_done, the number of anti-diagonals computed, at every residue of N_DONE_RESIDUES modulo 64: the odd ones where the sweep ends
    early, the even ones (no early end has them) where it runs to its end; both costs; at B > 64 also the deterministic ties"""
    evs, kms, wants = [], [], []
    cost, weights = R94D, (1.0, 1.0, 1.0)
    for res64 in N_DONE_RESIDUES:
        if res64 % 2:
            ev, km, w = case_of_n_done(checker, means, B, res64, cost, weights, end_in_last_block=res64 == 63)
            assert w["lo"].size < ev.size + km.size - 1
        else:
            ev, km = full_sweep_case(means, B, res64)
            w = checker.dtw(ev, km, cost, *weights, B)
            assert w["lo"].size == ev.size + km.size - 1
        assert w["lo"].size % 64 == res64 and w["end_row"] is not None and w["status"] in (OK, REF_END)
        evs.append(ev), kms.append(km), wants.append(w)
    assert {w["lo"].size % 16 for w in wants} >= {0, 1, 15}
    early = [(w, e.size) for w, e, k in zip(wants, evs, kms) if w["lo"].size < e.size + k.size - 1]
    assert len(early) == 4 and any(end_in_last_partial_block(w, cols) for w, cols in early), [(w["lo"].size, w["end_row"], c) for w, c in early]
    check(checker, batch(f"early end B {B}", evs, kms, cost, weights, B), lib=lib)
    check(checker, batch(f"early end B {B} r94p", evs, kms, R94P, (2.0, 1.0, 100.0), B), lib=lib)
    if B > 64:
        evs, kms, n_dones = zip(*[n_done_tie_case(means, B, c) for c in N_DONE_TIE_COLS])
        _, _, want = check(checker, batch(f"early end, ties, B {B}", evs, kms, R94P, (0.0, 0.0, 0.0), B), lib=lib)
        for w, n_done, e, k in zip(want, n_dones, evs, kms):
            assert w["lo"].size == n_done < e.size + k.size - 1 and w["end_row"] is not None
            assert np.array_equal(w["lo"], -B // 2 + np.arange(n_done) // 2)
        assert [n % 64 for n in n_dones] == [63, 1, 15]


def check_path_residues(checker, means, B, lib=None):
    """paths of 63, 64, 65 and 128 pairs, around the flush of 64 pairs, with two and four cells a lane, both costs and weight sets"""
    for cost in (R94P, R94D):
        for weights in WEIGHT_SETS:
            evs, kms = zip(*[case_of_path_len(checker, means, n, cost, weights, B) for n in (63, 64, 65, 128)])
            assert all(k.size == B + B // 2 for k in kms)
            _, _, want = check(checker, batch(f"path lengths B {B} cost {cost} weights {weights}", evs, kms, cost, weights, B), lib=lib)
            assert [w["path_len"] for w in want] == [63, 64, 65, 128]


def sweep_without_last_column(checker, means):
    """every shape of up to 40 x 40 at B = 64 with random events and with all-tie events, then taller shapes at every width with
    events that follow k-mers far down the stretch (the band runs ahead of the last column) -> the number of alignments for which no
    cell of the last column was computed, and the number looked at"""
    rng = np.random.default_rng(49)
    none = n = 0
    for rows in range(1, 41):
        km = rng.integers(0, 1024, rows).astype(np.uint16)
        for cols in range(1, 41):
            for ev, cost, weights in ((rng.uniform(60, 130, cols).astype(np.float32), R94D, (1.0, 1.0, 1.0)),
                                      (np.full(cols, 90, np.float32), R94P, (0.0, 0.0, 0.0))):
                none += checker.dtw(ev, km, cost, *weights, 64)["end_row"] is None
                n += 1
    for B in (64, 128, 256):
        for rows, cols, skip in ((2 * B, 5, B), (2 * B, 17, B), (3 * B, 40, 2 * B), (3 * B, 33, B), (B + 9, 3, B // 2 + 9)):
            km = rng.integers(0, 1024, rows).astype(np.uint16)
            for ev, cost, weights in ((dc.follow(rng, means, km[skip:skip + cols], cols, 0.5), R94D, (1.0, 1.0, 1.0)),
                                      (np.full(cols, 90, np.float32), R94P, (0.0, 0.0, 0.0))):
                for tall in (km, np.concatenate([km[:1], km])):
                    w = checker.dtw(ev, tall, cost, *weights, B)
                    none += w["end_row"] is None
                    n += 1
    return none, n


# ------------------------------------------------------------------ 2. events that are no numbers, and ties in every move
def nonfinite_batch(means, rows=150, cols=140, band=64, cost=R94D, weights=(1.0, 1.0, 1.0), seed=42, where="middle"):
    """one NaN, one +inf, one -inf event in an alignment of its own, in the middle (column cols // 2), at column 0 (the first load of
    events feeds (0, 0)) or at column cols - 1 (no score of the last column compares: the end cell is its last computed cell)"""
    rng = np.random.default_rng(seed)
    base, km = follow_case(rng, means, rows, cols)
    at = dict(middle=cols // 2, first=0, last=cols - 1)[where]
    evs = []
    for bad in (np.nan, np.inf, -np.inf):
        ev = base.copy()
        ev[at] = bad
        evs.append(ev)
    return batch(f"non-finite events, {where}", evs, [km] * 3, cost, weights, band)


NONFINITE_COMBOS = ((R94D, (1.0, 1.0, 1.0)), (R94P, (2.0, 1.0, 100.0)), (R94P, (0.0, 0.0, 0.0)), (R94D, (0.0, 0.0, 0.0)))


def check_nonfinite_ends(checker, means, lib=None):
    """non-finite events at column 0 and at column cols - 1, B = 64 and 128, the cost and weight combinations of the test of the
    middle column; then all-equal events with weights 1 at B = 256: the last column's ties go to the first smallest"""
    for B in (64, 128):
        for cost, weights in NONFINITE_COMBOS:
            for where in ("first", "last"):
                b = nonfinite_batch(means, band=B, cost=cost, weights=weights, where=where)
                _, _, want = check(checker, b, lib=lib)
                if where == "last":
                    # NaN in the last column: the end row is that of the column's last computed cell, on anti-diagonal n_done - 1
                    w, cols = want[0], b["evs"][0].size
                    assert np.isnan(w["score"]) and w["end_row"] == w["lo"].size - 1 - (cols - 1) >= max(0, int(w["lo"][-1])), (w["end_row"], w["lo"].size)
                    assert w["path"][0].tolist() == [cols - 1, w["end_row"]] or w["status"] == LEFT_BAND
    for cost in (R94D, R94P):
        b = all_equal_batch(means, rows=300, cols=140, band=256)
        b = batch("all-equal events B 256", b["evs"], b["kms"], cost, (1.0, 1.0, 1.0), 256)
        _, _, want = check(checker, b, lib=lib)
        for ev, km, w in zip(b["evs"], b["kms"], want):
            cells = checker.dtw(ev, km, cost, 1.0, 1.0, 1.0, 256, cells=True)["cells"]
            last = sorted((i, v) for (i, j), v in cells.items() if j == ev.size - 1)
            least = min(v for _, v in last)
            assert sum(v == least for _, v in last) >= 2 and w["end_row"] == next(i for i, v in last if v == least), (w["end_row"], last[:3])


def all_equal_batch(means, rows=150, cols=140, band=64):
    km = np.full(rows, 77, np.uint16)
    ev = np.full(cols, means[77], np.float32)
    return batch("all-equal events", [ev, ev], [km, km[:40]], R94D, (1.0, 1.0, 1.0), band)


# ------------------------------------------------------------------ 3. a band that binds
def long_skip_case(means, skip=100, seed=5):
    """two events per k-mer along 60 k-mers, then `skip` k-mers without an event, then 100 more k-mers: the full matrix's path runs
    `skip` rows down one column, which a band of 64 rows that moves one row an anti-diagonal does not hold"""
    rng = np.random.default_rng(seed)
    km = rng.integers(0, 1024, 400).astype(np.uint16)
    idx = np.concatenate([np.repeat(np.arange(60), 2), np.repeat(np.arange(60 + skip, 60 + skip + 100), 2)])
    ev = (means[km[idx]] + 0.5 * rng.standard_normal(idx.size)).astype(np.float32)
    return ev, km


def check_binding(checker, means, lib=None):
    ev, km = long_skip_case(means)
    weights = (1.0, 1.0, 1.0)
    full = checker.full(ev, km, R94D, *weights)
    want = checker.dtw(ev, km, R94D, *weights, 64, cells=True)
    outside = sum((int(i), int(j)) not in want["cells"] for j, i in full["path"])
    assert outside > 0 and want["status"] == OK and want["score"] > full["score"]      # the premise
    res, paths = run(batch("binding", [ev], [km], R94D, weights, 64), lib=lib)
    assert_equal_to_checker(res, paths, [want], "binding")
    assert res["score"][0] >= full["score"]


# ------------------------------------------------------------------ 4. the C ABI as a caller may use it
def check_argument_errors(lib):
    import pytest
    from uncalled_amd import capi
    ev, km = np.full(4, 90, np.float32), np.arange(4, dtype=np.uint16)
    res = np.zeros(1, capi.DTW_RESULT)
    off = np.array([0, 4], np.uint64)
    for subseq, band in ((dc.NONE, 0), (dc.NONE, 32), (dc.NONE, 96), (dc.NONE, 192), (dc.NONE, 512), (dc.ROW, 64), (dc.COL, 64)):
        prm = capi.DTWParams(subseq, R94D, 1, 1, 1)
        rc = lib.unc_dtw_adapt_batch(0, 1, ev.ctypes.data, off.ctypes.data, km.ctypes.data, off.ctypes.data, C.byref(prm), band, 0, res.ctypes.data,
                                     None, None, None)
        assert rc == -1, (subseq, band, rc)         # UNC_ERR_ARG
    for evs, kms, prm in (([ev[:0]], [km], capi.DTWParams(0, 0, 1, 1, 1)), ([ev], [km + 1021], capi.DTWParams(0, 0, 1, 1, 1)),
                          ([ev], [km], capi.DTWParams(3, 0, 1, 1, 1)), ([ev], [km], capi.DTWParams(0, 2, 1, 1, 1))):
        with pytest.raises(capi.UncalledHipError, match="error -1"):
            capi.dtw_batch(evs, kms, prm, lib=lib, adaptive=64)
    # the align pipeline refuses the same before anything runs
    raw = np.zeros(100, np.int16)
    calib = capi.make_calib(1, 1.0, 0.0, 8.0)
    for o in (capi.align_opts(create_events=False, adaptive=96), capi.align_opts(create_events=False, adaptive=128, dtw=capi.DTWParams(dc.ROW, R94D, 1, 1, 1))):
        with pytest.raises(capi.UncalledHipError, match="error -1"):
            capi.align_batch(raw, [0, raw.size], calib, [(0, 0, 0)], [km], opts=o, lib=lib)
    o = capi.AlignOpts()
    o.flags, o.band = capi.ALIGN_ADAPTIVE | capi.ALIGN_RAW, 0
    with pytest.raises(capi.UncalledHipError, match="error -1"):
        capi.align_batch(raw, [0, raw.size], calib, [(0, 0, 0)], [km], opts=o, lib=lib)


def check_caller_offsets(L, checker, means, band=64, device=0, seed=44):
    """unc_dtw_adapt_batch with ev_off[0] = 13, km_off[0] = 7, path_off[0] = 5, NaN events and 0xFFFF k-mers outside the batch's
    stretch, rooms for the paths of: the length + 3, the length, 5 short, 0, 1; sentinels around and between."""
    from uncalled_amd import capi
    rng = np.random.default_rng(seed)
    shape_list = [(70, 50), (33, 130), (64, 64), (20, 90), (90, 15)]
    cost, weights = R94P, (2.0, 1.0, 100.0)
    evs, kms = zip(*[follow_case(rng, means, r, c) for r, c in shape_list])
    want = [checker.dtw(e, k, cost, *weights, band) for e, k in zip(evs, kms)]
    assert all(w["status"] in (OK, REF_END) for w in want)
    need = [w["path_len"] for w in want]
    rooms = [need[0] + 3, need[1], need[2] - 5, 0, 1]
    assert need[2] > 5 and need[3] > 0 and need[4] > 1
    ev = np.concatenate([np.full(13, np.nan, np.float32)] + list(evs) + [np.full(9, np.nan, np.float32)])
    km = np.concatenate([np.full(7, 0xFFFF, np.uint16)] + list(kms) + [np.full(9, 0xFFFF, np.uint16)])
    ev_off = (13 + np.cumsum([0] + [e.size for e in evs])).astype(np.uint64)
    km_off = (7 + np.cumsum([0] + [k.size for k in kms])).astype(np.uint64)
    path_off = (5 + np.cumsum([0] + rooms)).astype(np.uint64)
    path = np.full((int(path_off[-1]) + 64, 2), SENTINEL, np.uint32)
    res = np.zeros(len(shape_list), capi.DTW_RESULT)
    prm = capi.DTWParams(dc.NONE, cost, *weights)
    rc = L.unc_dtw_adapt_batch(device, len(shape_list), ev.ctypes.data, ev_off.ctypes.data, km.ctypes.data, km_off.ctypes.data, C.byref(prm), band,
                               0, res.ctypes.data, path.ctypes.data, path_off.ctypes.data, None)
    assert rc == 0
    written = np.zeros(path.shape[0], bool)
    for a, w in enumerate(want):
        got = min(need[a], rooms[a])
        assert res["status"][a] == (w["status"] if rooms[a] >= need[a] else capi.DTW_PATH_TRUNCATED), a
        assert dc.bits(res["score"][a]) == w["score_bits"] and dc.bits(res["mean_score"][a]) == dc.bits(w["mean"]), a
        assert int(res["path_len"][a]) == need[a], a
        at = int(path_off[a])
        assert np.array_equal(path[at:at + got], w["path"][:got]), a
        written[at:at + got] = True
    assert (path[~written] == SENTINEL).all()
    # no alignments: accepted, nothing to do, and the timing says so
    ms, rounds, held = C.c_float(1), C.c_uint32(1), C.c_uint64(1)
    rc = L.unc_dtw_adapt_batch(device, 0, ev.ctypes.data, ev_off.ctypes.data, km.ctypes.data, km_off.ctypes.data, C.byref(prm), band, 0,
                               res.ctypes.data, None, None, None)
    assert rc == 0
    L.unc_dtw_last_timing(C.byref(ms), C.byref(rounds), C.byref(held))
    assert (ms.value, rounds.value, held.value) == (0.0, 0, 0)


def rounds_batch(means, n=12, seed=45):
    """12 alignments of about 100 x 150 at B = 64 and a workspace that holds four of them"""
    rng = np.random.default_rng(seed)
    shape_list = [(100 + 3 * a, 150 - 2 * a) for a in range(n)]
    evs, kms = zip(*[follow_case(rng, means, r, c) for r, c in shape_list])
    b = batch("rounds", evs, kms, R94D, (1.0, 1.0, 1.0), 64)
    sizes = [adapt_crumb_bytes(r, c, 64) for r, c in shape_list]
    b["workspace"] = sum(sorted(sizes)[-4:])
    b["sizes"] = sizes
    return b


def check_rounds_and_too_large(checker, means, lib=None):
    from uncalled_amd import capi
    b = rounds_batch(means)
    res0, paths0, want = check(checker, b, lib=lib)
    ms, rounds, held = capi.dtw_last_timing(lib)
    assert rounds == 1 and held == sum(b["sizes"])
    res1, paths1 = run(b, lib=lib, workspace_bytes=b["workspace"])
    ms, rounds, held = capi.dtw_last_timing(lib)
    assert rounds >= 3 and held <= b["workspace"], (rounds, held)
    assert_equal_to_checker(res1, paths1, want, "rounds")
    # one alignment too large for the workspace: reported, the others computed
    sizes = b["sizes"] + [adapt_crumb_bytes(400, 400, 64)]
    rng = np.random.default_rng(46)
    ev, km = follow_case(rng, means, 400, 400)
    big = batch("too large", b["evs"] + [ev], b["kms"] + [km], b["cost"], b["weights"], 64)
    assert sizes[-1] > max(sizes[:-1])
    res, paths = run(big, lib=lib, workspace_bytes=sizes[-1] - 1)
    assert res["status"][-1] == capi.DTW_TOO_LARGE and res["path_len"][-1] == 0 and res["score"][-1] == 0 and paths[-1] is None
    assert_equal_to_checker(res[:-1], paths[:-1], want, "too large")


# ------------------------------------------------------------------ 5. the pipeline on the committed example read
EXAMPLE_STRETCHES = [(0, 6700, 7150, True), (0, 6550, 7000, False)]     # the slice's 300 bases and half as many again, either strand


def check_pipeline(G, X, checker, band=128):
    """align_ref_batch with adaptive=128 on a slice of the example read against a stretch 1.5 times too long, both strands: status,
    score and path are the checker's on the returned levels and k-mers; the segments are tests/segments_check.c's of that path and
    the returned events; the pile-up is the naive pile-up of those segments.  -> the results"""
    import pileup_cases as pc
    import segments_cases as sc
    from uncalled_amd import capi
    r = len(G.signals) - 1
    qs = [(r, 10001, 14001)] * len(EXAMPLE_STRETCHES)
    o = capi.align_opts(adaptive=band)
    pu = X.pileup()
    res, levs, paths, kms, segs, info, events = capi.align_ref_batch(X.refseq, G.raw, G.offsets, G.calib, qs, EXAMPLE_STRETCHES, o, levels=True,
                                                                     paths=True, kmers=True, segments=True, events=True, pileup=pu)
    segck = sc.SegChecker()
    for q in range(len(qs)):
        w = checker.dtw(levs[q], kms[q], R94D, 1.0, 1.0, 1.0, band)
        assert w["status"] in (OK, REF_END) and int(res["status"][q]) == w["status"], (q, res["status"][q], w["status"])
        assert same_float(res["dtw"]["score"][q], w["score"]) and same_float(res["dtw"]["mean_score"][q], w["mean"]), q
        assert np.array_equal(paths[q], w["path"]), q
        want_seg, row_first = segck.segments(w["path"], events[q], np.arange(events[q].size, dtype=np.uint32), qs[q][1], res["scale"][q],
                                             res["shift"][q])
        assert int(info["status"][q]) == capi.SEG_OK and int(info["row_first"][q]) == row_first == 0
        assert int(info["n_rows"][q]) == want_seg.size == int(w["path"][0][1]) + 1 and sc.rec_equal(segs[q], want_seg), q
    nv = pc.naive_of_segments(pc.whole(X), EXAMPLE_STRETCHES, segs, info)
    assert nv.added > 100
    pc.equals_naive(pu, nv)
    # without the flag the same options are the fixed band of the same width: another alignment, the old statuses
    fixed = capi.align_ref_batch(X.refseq, G.raw, G.offsets, G.calib, qs, EXAMPLE_STRETCHES, capi.align_opts(band=band))
    assert (fixed["status"] == capi.DTW_OK).all() and fixed["dtw"].tobytes() != res["dtw"].tobytes()
    return res
