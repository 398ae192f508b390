"""TEST INFRASTRUCTURE: the DTW cases that tests/test_dtw_cpu.py (k_dtw.hip under the lanesim emulator, small sizes) and
tests/test_gpu_dtw.py (the gfx950 library, full sizes) share, and the one comparison both make: bits of score, bits of mean_score,
path_len, status and the whole path against Checker.dtw (tests/dtw_check.c).

A batch is a dict: name, evs, kms (one array per alignment), subseq, cost, weights (one parameter set: a batch is one call), and
`of`: for every alignment the index of its distinct case, so that the checker runs once per distinct case however often the batch
repeats it.  Builders take `means`, the library's model means (capi.dtw_model_tables()[0]); all are seeded."""
import ctypes as C

import numpy as np

NONE, ROW, COL = 0, 1, 2
R94P, R94D = 0, 1
COMBOS = [(s, c) for s in (NONE, ROW, COL) for c in (R94P, R94D)]
WEIGHTS = {NONE: (2.0, 1.0, 100.0), ROW: (10.0, 1.0, 1000.0), COL: (1.0, 1.0, 1.0)}      # one set of weights per mode
SENTINEL = 0xDEADBEEF


def crumb_bytes(rows, cols):
    """bytes of back-pointers the library holds for one alignment (dtw_crumb_words of dtw_dev.h, times 4)"""
    return 4 * 64 * ((rows + 63) // 64) * ((cols + 63 + 15) // 16)


def bits(x):
    return int(np.asarray(x, np.float32).reshape(-1)[:1].view(np.uint32)[0])


def assert_equal_to_checker(res, paths, want, skip=()):
    from uncalled_amd import capi
    compared = 0
    for a, w in enumerate(want):
        if a in skip:
            continue
        assert res["status"][a] == capi.DTW_OK, a
        assert bits(res["score"][a]) == w["score_bits"], (a, res["score"][a], w["score"])
        assert bits(res["mean_score"][a]) == bits(w["mean"]), a
        assert int(res["path_len"][a]) == w["path_len"], a
        if paths is not None:
            assert paths[a].shape == w["path"].shape and np.array_equal(paths[a], w["path"]), a
        compared += 1
    assert compared == len(want) - len(skip)


def batch(name, evs, kms, subseq, cost, weights=None, of=None, **more):
    assert len(evs) == len(kms)
    return dict(name=name, evs=list(evs), kms=list(kms), subseq=subseq, cost=cost, weights=WEIGHTS[subseq] if weights is None else weights,
                of=list(range(len(evs))) if of is None else list(of), **more)


def params(b):
    from uncalled_amd import capi
    return capi.DTWParams(b["subseq"], b["cost"], *b["weights"])


def wanted(checker, b):
    """the checker's result of every alignment of the batch (one run per distinct case)"""
    first = {}
    for a, d in enumerate(b["of"]):
        first.setdefault(d, a)
    done = {d: checker.dtw(b["evs"][a], b["kms"][a], b["subseq"], b["cost"], *b["weights"]) for d, a in first.items()}
    return [done[d] for d in b["of"]]


def run(b, lib=None, **kw):
    from uncalled_amd import capi
    return capi.dtw_batch(b["evs"], b["kms"], params(b), lib=lib, full=True, **kw)


def check(checker, b, lib=None, **kw):
    """run the batch, hold every alignment against the checker -> (res, paths, want)"""
    want = wanted(checker, b)
    res, paths = run(b, lib=lib, **kw)
    assert_equal_to_checker(res, paths, want)
    return res, paths, want


def follow(rng, means, km, cols, noise=1.5):
    """events that follow the k-mers' model means with stays, skips and noise"""
    return (means[km[np.sort(rng.integers(0, km.size, cols))]] + noise * rng.standard_normal(cols)).astype(np.float32)


# ------------------------------------------------------------------ 1. more alignments than wavefronts
def queue_batches(means, n, n_distinct, max_side, seed=1):
    """n alignments cycling n_distinct small cases from 1 x 1 to max_side x max_side, once per subseq x cost"""
    rng = np.random.default_rng(seed)
    shapes = [(1, 1), (1, max_side), (max_side, 1), (max_side, max_side), (2, 1), (1, 2)]
    shapes += [(r, c) for r, c in ((64, 64), (65, 63), (63, 65), (128, 17), (17, 128), (129, 129)) if max(r, c) <= max_side]
    while len(shapes) < n_distinct:
        shapes.append((int(rng.integers(1, max_side + 1)), int(rng.integers(1, max_side + 1))))
    shapes = shapes[:n_distinct]
    evs, kms = [], []
    for d, (rows, cols) in enumerate(shapes):
        km = rng.integers(0, 1024, rows).astype(np.uint16)
        kms.append(km)
        evs.append(rng.uniform(60, 130, cols).astype(np.float32) if d % 3 == 2 else follow(rng, means, km, cols))
    of = [a % n_distinct for a in range(n)]
    return [batch(f"queue subseq {s} cost {c}", [evs[d] for d in of], [kms[d] for d in of], s, c, of=of) for s, c in COMBOS]


# ------------------------------------------------------------------ 2. row and column indices past 2^16
LONG_SHAPES = [(70000, 300, 67000), (300, 70000, 67000), (66000, 1, 65800), (1, 66000, 65800), (65537, 17, 65520)]      # rows, cols, at


def long_index_batches(means, shapes=LONG_SHAPES, seed=2):
    """One batch per subseq mode, r94p and r94d in turn.  The short side follows the stretch of the long side that starts at `at`
    (a single event lies exactly on the mean of a k-mer that occurs only there, a single k-mer's mean is one event there), so
    that DTWSubSeq::ROW on a tall matrix and ::COL on a wide one put the whole path past index 2^16."""
    rng = np.random.default_rng(seed)
    evs, kms = [], []
    for rows, cols, at in shapes:
        assert at + min(rows, cols) <= max(rows, cols)
        if rows >= cols:
            km = rng.integers(0, 1023, rows).astype(np.uint16)
            if cols == 1:
                km[at] = 1023
                ev = means[km[at:at + 1]].copy()
            else:
                ev = (means[km[at:at + cols]] + 0.3 * rng.standard_normal(cols)).astype(np.float32)
        else:
            km = rng.integers(0, 1024, rows).astype(np.uint16)
            ev = rng.uniform(60, 130, cols).astype(np.float32)
            if rows == 1:
                ev[np.abs(ev - means[km[0]]) < 0.5] += np.float32(1.0)       # (no other event near enough to cost the same in floats)
                ev[at] = means[km[0]]
            else:
                ev[at:at + rows] = (means[km] + 0.3 * rng.standard_normal(rows)).astype(np.float32)
        evs.append(ev); kms.append(km)
    return [batch(f"long subseq {s}", evs, kms, s, (R94P, R94D)[s & 1], at=[x[2] for x in shapes]) for s in (NONE, ROW, COL)]


def assert_long_indices_used(b, want):
    """the premise of long_index_batches: the paths the checker expects do hold indices of 2^16 and more"""
    for a, w in enumerate(want):
        rows, cols, at = b["kms"][a].size, b["evs"][a].size, b["at"][a]
        end, start = w["path"][0], w["path"][-1]          # (event j, k-mer i)
        assert max(rows, cols) > 65536
        if b["subseq"] == NONE:
            assert tuple(end) == (cols - 1, rows - 1) and tuple(start) == (0, 0) and w["path_len"] >= max(rows, cols), a
        elif (b["subseq"] == ROW and rows > cols) or (b["subseq"] == COL and cols > rows):
            x = 1 if b["subseq"] == ROW else 0
            assert end[x] >= 65536 and abs(int(end[x]) - (at + min(rows, cols) - 1)) <= 8 and abs(int(start[x]) - at) <= 8, (a, end, start)
            assert start[x] >= 65536 or at < 65536, (a, start)


# ------------------------------------------------------------------ 3. more than 4 GiB of back-pointers in one round
BIG_SHAPES = [(6000, 4000), (5990, 4010), (6010, 3990), (5960, 4030)]


def big_round_batch(means, n=720, shapes=BIG_SHAPES, subseq=NONE, cost=R94P, seed=3):
    rng = np.random.default_rng(seed)
    kms = [rng.integers(0, 1024, r).astype(np.uint16) for r, _ in shapes]
    evs = [follow(rng, means, km, c) for km, (_, c) in zip(kms, shapes)]
    of = [a % len(shapes) for a in range(n)]
    b = batch("big round", [evs[d] for d in of], [kms[d] for d in of], subseq, cost, of=of)
    b["workspace"] = sum(crumb_bytes(k.size, e.size) for e, k in zip(b["evs"], b["kms"]))
    return b


# ------------------------------------------------------------------ 4. offsets as a caller may give them
def check_caller_offsets(L, checker, means, device=0, seed=4):
    """The raw C ABI with ev_off[0] = 13, km_off[0] = 7, path_off[0] = 5, NaN events and 0xFFFF k-mers outside the batch's stretch,
    and rooms for the paths of: the length + 3, the length, 5 short, 0, more than rows + cols - 1, 1.  Every word of the path
    buffer outside [path_off[a], path_off[a] + min(path_len, room)) must keep its sentinel."""
    from uncalled_amd import capi
    rng = np.random.default_rng(seed)
    shapes = [(70, 50), (33, 130), (64, 64), (20, 90), (1, 1), (90, 5)]
    for subseq, cost in ((ROW, R94D), (NONE, R94P), (COL, R94P)):
        kms = [rng.integers(0, 1024, r).astype(np.uint16) for r, _ in shapes]
        evs = [follow(rng, means, km, c) for km, (_, c) in zip(kms, shapes)]
        want = [checker.dtw(e, k, subseq, cost, *WEIGHTS[subseq]) for e, k in zip(evs, kms)]
        need = [w["path_len"] for w in want]
        rooms = [need[0] + 3, need[1], need[2] - 5, 0, shapes[4][0] + shapes[4][1] - 1 + 10, 1]
        assert need[2] > 5 and need[3] > 0 and need[5] > 1
        ev = np.concatenate([np.full(13, np.nan, np.float32)] + evs + [np.full(9, np.nan, np.float32)])
        km = np.concatenate([np.full(7, 0xFFFF, np.uint16)] + kms + [np.full(9, 0xFFFF, np.uint16)])
        ev_off = (13 + np.cumsum([0] + [e.size for e in evs])).astype(np.uint64)
        km_off = (7 + np.cumsum([0] + [k.size for k in kms])).astype(np.uint64)
        path_off = (5 + np.cumsum([0] + rooms)).astype(np.uint64)
        path = np.full((int(path_off[-1]) + 64, 2), SENTINEL, np.uint32)
        res = np.zeros(len(shapes), capi.DTW_RESULT)
        prm = capi.DTWParams(subseq, cost, *WEIGHTS[subseq])
        rc = L.unc_dtw_batch(device, len(shapes), ev.ctypes.data, ev_off.ctypes.data, km.ctypes.data, km_off.ctypes.data, C.byref(prm), 0,
                             res.ctypes.data, path.ctypes.data, path_off.ctypes.data, None)
        assert rc == 0
        written = np.zeros(path.shape[0], bool)
        for a, w in enumerate(want):
            got = min(need[a], rooms[a])
            assert res["status"][a] == (capi.DTW_OK if rooms[a] >= need[a] else capi.DTW_PATH_TRUNCATED), (subseq, a)
            assert bits(res["score"][a]) == w["score_bits"] and bits(res["mean_score"][a]) == bits(w["mean"]), (subseq, a)
            assert int(res["path_len"][a]) == need[a], (subseq, a)
            at = int(path_off[a])
            assert np.array_equal(path[at:at + got], w["path"][:got]), (subseq, a)
            written[at:at + got] = True
        assert (path[~written] == SENTINEL).all(), (subseq, np.flatnonzero((path[~written] != SENTINEL).any(axis=1)))
        assert not (path[written] == SENTINEL).all(axis=1).any()

    # no alignments: nothing to do, and the timing says so
    ms, rounds, held = C.c_float(1), C.c_uint32(1), C.c_uint64(1)
    rc = L.unc_dtw_batch(device, 0, ev.ctypes.data, ev_off.ctypes.data, km.ctypes.data, km_off.ctypes.data, C.byref(prm), 0, res.ctypes.data,
                         None, None, None)
    assert rc == 0
    L.unc_dtw_last_timing(C.byref(ms), C.byref(rounds), C.byref(held))
    assert (ms.value, rounds.value, held.value) == (0.0, 0, 0)


def check_no_paths_with_a_too_large_member(checker, means, lib=None, seed=5):
    """paths=False with a workspace one byte short of the largest alignment: that one is reported, the others' scores are right"""
    from uncalled_amd import capi
    rng = np.random.default_rng(seed)
    shapes = [(40, 30), (130, 120), (64, 64), (10, 100)]
    kms = [rng.integers(0, 1024, r).astype(np.uint16) for r, _ in shapes]
    evs = [follow(rng, means, km, c) for km, (_, c) in zip(kms, shapes)]
    b = batch("too large", evs, kms, COL, R94D)
    sizes = [crumb_bytes(r, c) for r, c in shapes]
    big = int(np.argmax(sizes))
    assert sorted(sizes)[-2] < sizes[big] - 1
    res, paths = run(b, lib=lib, paths=False, workspace_bytes=sizes[big] - 1)
    assert paths is None
    assert res["status"][big] == capi.DTW_TOO_LARGE and res["path_len"][big] == 0 and res["score"][big] == 0
    assert_equal_to_checker(res, None, wanted(checker, b), skip=(big,))


# ------------------------------------------------------------------ 5. ties at the end cell
def end_tie_batches(means, big_reps=70, seed=6):
    """r94d with events exactly on model means: a unit of 37 k-mers of distinct means against itself costs 0 along the diagonal.
    ROW: the k-mers are the unit `reps` times over, the events the unit's means: the last column holds an exact 0 wherever a
    repeat ends (rows 36, 73, ...: lanes 36, 9, 46, 19, 56, 29 of four strips at 6 repeats; at 70 repeats every lane meets
    several).  As built the last cell is one of them and the end cell stays there (dtw.hpp:81-85: only a strictly smaller score
    moves it); with 5 k-mers of other means appended the last cell is larger and the end cell is the FIRST zero, row 36 -- not
    row 73 of the smaller lane 9.  COL: the mirror image.  `end`[a] is the (event, k-mer) the path must start with."""
    rng = np.random.default_rng(seed)
    order = rng.permutation(1024)
    unit, seen = [], set()
    for k in order:
        if float(means[k]) not in seen and len(unit) < 37:
            unit.append(int(k)); seen.add(float(means[k]))
    unit = np.array(unit, np.uint16)
    others = np.array([k for k in order if float(means[k]) not in seen][:5], np.uint16)      # (no mean of the unit's)
    assert unit.size == 37 and others.size == 5
    out = []
    for subseq in (ROW, COL):
        evs, kms, end, last = [], [], [], []
        for reps in (6, big_reps):
            for extra in (False, True):
                long_k = np.concatenate([np.tile(unit, reps), others]) if extra else np.tile(unit, reps)
                if subseq == ROW:
                    kms.append(long_k); evs.append(means[unit].copy())
                    end.append((36, 36) if extra else (36, long_k.size - 1))
                else:
                    kms.append(unit.copy()); evs.append(means[long_k].copy())
                    end.append((36, 36) if extra else (long_k.size - 1, 36))
                last.append(not extra)
        for weights in sorted({WEIGHTS[subseq], (1.0, 1.0, 1.0), (2.0, 1.0, 100.0)}):
            out.append(batch(f"end ties subseq {subseq} weights {weights}", evs, kms, subseq, R94D, weights=weights, end=end, last_is_min=last,
                             min_cells=[6, 6, big_reps, big_reps]))
    return out


def assert_end_ties(b, want):
    """the premise of end_tie_batches, from the checker's own counters"""
    for a, w in enumerate(want):
        assert w["score"] == 0.0 and w["end_min_cells"] >= b["min_cells"][a] and w["last_is_min"] == b["last_is_min"][a], (b["name"], a, w)
        assert tuple(int(x) for x in w["path"][0]) == b["end"][a], (b["name"], a, w["path"][0])


# ------------------------------------------------------------------ 6. ties in every cell, and events that are no numbers
def zero_weight_batches(means, rows, cols, seed=7):
    """dw = hw = vw = 0: every score is 0 (or the border's MAX_COST), every comparison a tie"""
    rng = np.random.default_rng(seed)
    km = rng.integers(0, 1024, rows).astype(np.uint16)
    ev = follow(rng, means, km, cols)
    return [batch(f"zero weights subseq {s}", [ev], [km], s, (R94P, R94D, R94P)[s], weights=(0.0, 0.0, 0.0)) for s in (NONE, ROW, COL)]


def rounded_batches(means, rows, cols, step, seed=8):
    """r94d, weights (1, 1, 1), events rounded to multiples of `step`: equal events give equal columns of costs, and with equal
    weights equal sums of them"""
    rng = np.random.default_rng(seed)
    km = rng.integers(0, 1024, rows).astype(np.uint16)
    ev = (np.round(follow(rng, means, km, cols) / step) * step).astype(np.float32)
    return [batch(f"rounded events subseq {s}", [ev], [km], s, R94D, weights=(1.0, 1.0, 1.0)) for s in (NONE, ROW, COL)]


def nonfinite_batches(means, rows, cols, seed=9):
    """one NaN, one +inf, one -inf event, in the middle of the alignment and at column 5 (the first column of its lane in the COL
    scan of the last row), each in an alignment of its own.  The reference's comparisons (dtw.hpp:62-71, 82, 89) are well
    defined on them: a NaN is never <= or <, so it falls through to V and is never chosen as the end cell."""
    rng = np.random.default_rng(seed)
    km = rng.integers(0, 1024, rows).astype(np.uint16)
    base = follow(rng, means, km, cols)
    evs = []
    for at in (cols // 2, 5):
        for bad in (np.nan, np.inf, -np.inf):
            ev = base.copy()
            ev[at] = bad
            evs.append(ev)
    return [batch(f"non-finite events subseq {s}", evs, [km] * len(evs), s, (R94D, R94P, R94D)[s]) for s in (NONE, ROW, COL)] + \
           [batch(f"non-finite events, weights 0, subseq {s}", evs, [km] * len(evs), s, R94P, weights=(0.0, 0.0, 0.0)) for s in (ROW, COL)]


def nan_before_the_end_batch(means, rows=100, cols=200, at=10):
    """DTWSubSeq::COL, r94d: a NaN event at column 5, then events exactly on the k-mers' means from column `at` on: the last row's
    only 0 lies at column at + rows - 1 (109: lane 45 of the second block of 64), its cell at column 5 is NaN.  The reference's
    scan (dtw.hpp:88-92) passes over the NaN; a scan that lets a lane's FIRST cell stand as its candidate keeps it in lane 5, and
    no comparison in a butterfly reduction ever replaces it, so the lanes it is exchanged with lose what it should have carried."""
    rng = np.random.default_rng(10)
    km = rng.integers(0, 1024, rows).astype(np.uint16)
    ev = rng.uniform(60, 130, cols).astype(np.float32)
    ev[at:at + rows] = means[km]
    ev[5] = np.nan
    return batch("NaN before the end cell", [ev], [km], COL, R94D, weights=(2.0, 1.0, 100.0), end=[(at + rows - 1, rows - 1)])
