"""GPU: unc_dtw_batch (k_dtw.hip) against the reference's committed results (tests/golden/dtw_goldens.npz, bit for bit) and, for
sizes the goldens cannot hold, against the CPU checker (tests/dtw_check.c), which reproduces every golden (tests/test_dtw_cpu.py).
The cases past the goldens' reach come from tests/dtw_cases.py, which tests/test_dtw_cpu.py runs in small under the emulator.
Measured on an MI355X box (profiles/dtw_tests_first_run.txt): the file takes 8.5 s, 3 s of it the CPU checker on the mixed batch
(6 x 68 M cells), 1.3 s the indices past 2^16 and 1.0 s the 4 GiB round (their checker runs above all).  The 4 GiB round: 720
alignments near 6000 x 4000, kernel 95.8 ms (one such alignment alone: 88 ms), 1 round, 4 413 818 880 bytes of back-pointers held:
byte quantities past 2^32, word offsets (DtwJob::crumb_off) not."""
import numpy as np
import pytest

import dtw_cases as dc
from conftest import EX_PREFIX, GOLD
from dtw_cases import COMBOS, WEIGHTS, assert_equal_to_checker, crumb_bytes
from dtw_check import Checker

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD / "dtw_goldens.npz")


@pytest.fixture(scope="module")
def checker():
    return Checker()


def gold_case(gold, a):
    from uncalled_amd import capi
    ev = gold["events"][int(gold["ev_off"][a]):int(gold["ev_off"][a + 1])]
    km = gold["kmers"][int(gold["km_off"][a]):int(gold["km_off"][a + 1])]
    prm = capi.DTWParams(int(gold["subseq"][a]), int(gold["cost"][a]), *map(float, gold["weights"][a]))
    path = gold["path"][int(gold["path_off"][a]):int(gold["path_off"][a + 1])].astype(np.uint32)
    return ev, km, prm, path


@pytest.fixture(scope="module")
def means(checker):
    return checker.model[:1024]


@pytest.fixture(scope="module")
def mixed():
    """72 alignments from 1 x 1 to 6000 x 4000 (rows = k-mers, cols = events): events follow the k-mers' model means with stays,
    skips and noise, or are unrelated to them."""
    from uncalled_amd import capi
    rng = np.random.default_rng(94)
    means = capi.dtw_model_tables()[0]
    shapes = [(6000, 4000), (3000, 4500), (2500, 2000), (1, 1), (1, 300), (300, 1), (64, 64), (65, 1000), (1000, 65), (63, 17)]
    shapes += [(int(r), int(c)) for r, c in zip(rng.integers(2, 1200, 62), rng.integers(2, 1200, 62))]
    evs, kms = [], []
    for n, (rows, cols) in enumerate(shapes):
        km = rng.integers(0, 1024, rows).astype(np.uint16)
        if n % 3 == 2:
            ev = rng.uniform(60, 130, cols).astype(np.float32)
        else:
            ev = (means[km[np.sort(rng.integers(0, rows, cols))]] + 1.5 * rng.standard_normal(cols)).astype(np.float32)
        evs.append(ev); kms.append(km)
    assert len(evs) >= 64
    return evs, kms


@pytest.fixture(scope="module")
def mixed_want(mixed, checker):
    evs, kms = mixed
    return {(s, c): [checker.dtw(e, k, s, c, *WEIGHTS[s]) for e, k in zip(evs, kms)] for s, c in COMBOS}


def test_every_golden_through_the_c_abi(hip_lib, gold):
    from uncalled_amd import capi
    for a in range(gold["subseq"].size):
        ev, km, prm, want = gold_case(gold, a)
        res, paths = capi.dtw_batch([ev], [km], prm, full=True)
        assert res["status"][0] == capi.DTW_OK
        assert int(res["score"].view(np.uint32)[0]) == int(gold["score_bits"][a]), a
        assert int(res["mean_score"].view(np.uint32)[0]) == int(gold["mean_bits"][a]), a
        assert int(res["path_len"][0]) == want.shape[0] and np.array_equal(paths[0], want), a


def test_every_golden_in_batches(hip_lib, gold):
    """the goldens of one parameter set share a launch"""
    from uncalled_amd import capi
    groups = {}
    for a in range(gold["subseq"].size):
        groups.setdefault((int(gold["subseq"][a]), int(gold["cost"][a]), tuple(map(float, gold["weights"][a]))), []).append(a)
    for (s, c, w), members in groups.items():
        cases = [gold_case(gold, a) for a in members]
        res, paths = capi.dtw_batch([x[0] for x in cases], [x[1] for x in cases], capi.DTWParams(s, c, *w), full=True)
        assert np.array_equal(res["score"].view(np.uint32), gold["score_bits"][members])
        assert np.array_equal(res["mean_score"].view(np.uint32), gold["mean_bits"][members])
        for p, x in zip(paths, cases):
            assert np.array_equal(p, x[3])


def test_every_golden_through_the_host_module(hip_lib, gold):
    from uncalled_amd import _uncalled_amd as m
    assert (m.DTW_EVENT_GLOB.dw, m.DTW_EVENT_GLOB.hw, m.DTW_EVENT_GLOB.vw) == (2.0, 1.0, 100.0)
    assert (m.DTW_RAW_GLOB.dw, m.DTW_RAW_GLOB.vw) == (10.0, 1000.0)
    assert (m.DTW_RAW_QSUB.dw, m.DTW_RAW_QSUB.subseq, m.DTW_RAW_RSUB.dw, m.DTW_RAW_RSUB.subseq) == (2.0, 2, 2.0, 1)   # the reference's aliasing
    for a in range(gold["subseq"].size):
        ev, km, prm, want = gold_case(gold, a)
        p = m.DTWParams()
        p.subseq, p.dw, p.hw, p.vw = prm.subseq, prm.dw, prm.hw, prm.vw
        d = (m.DTWr94d if prm.cost else m.DTWr94p)(ev.tolist(), km.tolist(), p)
        assert int(np.float32(d.score()).view(np.uint32)) == int(gold["score_bits"][a]), a
        assert int(np.float32(d.mean_score()).view(np.uint32)) == int(gold["mean_bits"][a]), a
        assert np.array_equal(np.array(d.get_path(), dtype=np.uint32).reshape(-1, 2), want), a


@pytest.mark.parametrize("subseq,cost", COMBOS)
def test_mixed_batch_equals_the_checker(hip_lib, mixed, mixed_want, subseq, cost):
    from uncalled_amd import capi
    evs, kms = mixed
    res, paths = capi.dtw_batch(evs, kms, capi.DTWParams(subseq, cost, *WEIGHTS[subseq]), full=True)
    ms, rounds, held = capi.dtw_last_timing()
    cells = sum(e.size * k.size for e, k in zip(evs, kms))
    print(f"mixed batch subseq {subseq} cost {cost}: {cells} cells, kernel {ms:.2f} ms, {cells / ms / 1e6:.1f} Gcells/s, {rounds} round(s), "
          f"{held / cells * 8:.3f} bits/cell")
    assert rounds == 1
    assert_equal_to_checker(res, paths, mixed_want[(subseq, cost)])


@pytest.mark.parametrize("subseq,cost", [(0, 0), (1, 1), (2, 0)])
def test_small_workspace_runs_in_rounds_with_identical_results(hip_lib, mixed, mixed_want, subseq, cost):
    from uncalled_amd import capi
    evs, kms = mixed
    biggest = max(crumb_bytes(k.size, e.size) for e, k in zip(evs, kms))
    total = sum(crumb_bytes(k.size, e.size) for e, k in zip(evs, kms))
    assert total > 2 * biggest
    res, paths = capi.dtw_batch(evs, kms, capi.DTWParams(subseq, cost, *WEIGHTS[subseq]), workspace_bytes=biggest, full=True)
    _, rounds, held = capi.dtw_last_timing()
    assert rounds >= 3 and held <= biggest
    assert_equal_to_checker(res, paths, mixed_want[(subseq, cost)])


def test_alignment_larger_than_the_workspace_is_reported(hip_lib, mixed, mixed_want):
    from uncalled_amd import capi
    evs, kms = mixed
    sizes = [crumb_bytes(k.size, e.size) for e, k in zip(evs, kms)]
    big = int(np.argmax(sizes))
    res, paths = capi.dtw_batch(evs, kms, capi.DTWParams(1, 0, *WEIGHTS[1]), workspace_bytes=sizes[big] - 1, full=True)
    assert res["status"][big] == capi.DTW_TOO_LARGE and paths[big] is None and res["path_len"][big] == 0
    assert sorted(sizes)[-2] < sizes[big] - 1
    assert_equal_to_checker(res, paths, mixed_want[(1, 0)], skip=(big,))


def test_no_paths_gives_the_same_scores(hip_lib, mixed, mixed_want):
    from uncalled_amd import capi
    evs, kms = mixed
    res, paths = capi.dtw_batch(evs, kms, capi.DTWParams(2, 1, *WEIGHTS[2]), paths=False, full=True)
    assert paths is None
    assert_equal_to_checker(res, None, mixed_want[(2, 1)])


def test_short_path_room_is_reported_not_overrun(hip_lib, gold):
    """the C ABI with room for fewer pairs than the path has: the pairs that fit, the full length, a status -- and nothing behind"""
    import ctypes as C
    from uncalled_amd import capi
    L = capi.load()
    a = int(np.argmax(gold["path_off"][1:] - gold["path_off"][:-1]))
    ev, km, prm, want = gold_case(gold, a)
    room = 37
    ev_off, km_off = np.array([0, ev.size], np.uint64), np.array([0, km.size], np.uint64)
    path_off = np.array([0, room], np.uint64)
    path = np.full((room + 64, 2), 0xDEADBEEF, np.uint32)
    res = np.zeros(1, capi.DTW_RESULT)
    rc = L.unc_dtw_batch(0, 1, ev.ctypes.data, ev_off.ctypes.data, km.ctypes.data, km_off.ctypes.data, C.byref(prm), 0, res.ctypes.data,
                         path.ctypes.data, path_off.ctypes.data, None)
    assert rc == 0 and res["status"][0] == capi.DTW_PATH_TRUNCATED and int(res["path_len"][0]) == want.shape[0]
    assert int(res["score"].view(np.uint32)[0]) == int(gold["score_bits"][a])
    assert np.array_equal(path[:room], want[:room]) and (path[room:] == 0xDEADBEEF).all()


def test_example_read_against_the_place_it_mapped(hip_lib, example, goldens, checker):
    """the read's normalised event means (unc_detect_events) against the k-mers of the stretch the reference maps it to: the mapped
    strand scores lower than the other one, and both equal the checker"""
    from uncalled_amd import capi
    hit = dict(zip([str(x) for x in goldens["hit_fields"]], [int(v) for v in goldens["ex_hit"]]))
    assert hit["mapped"]
    ix = capi.Index(EX_PREFIX, device=0)
    m = capi.Mapper(ix, n_slots=64)
    raw = example["signal"]
    cal = capi.make_calib(1, example["range"], example["offset"], example["digitisation"])
    means, moff, info = m.detect_events(raw, np.array([0, raw.size], np.uint64), cal)
    # the events of the mapped part of the read: the mapper had seen event_i events when it decided, PAF columns 3-4 (rd_st, rd_en,
    # in bases at a constant number of bases per event) say where in them the mapping lies
    ev = means[int(round(hit["event_i"] * hit["rd_st"] / hit["rd_en"])):hit["event_i"]]
    assert 30 < ev.size < hit["event_i"]
    st, en = hit["rf_st"], hit["rf_en"] + 1           # PAF columns 8-9, the end inclusive
    strands = {fwd: capi.ref_kmers(ix, EX_PREFIX, 0, st, en, fwd) for fwd in (True, False)}
    assert strands[True].size == en - st - 4
    for prm in (capi.DTW_EVENT_RSUB, capi.DTW_EVENT_QSUB):
        res, paths = capi.dtw_batch([ev, ev], [strands[True], strands[False]], prm, full=True)
        for a, fwd in enumerate((True, False)):
            w = checker.dtw(ev, strands[fwd], prm.subseq, prm.cost, prm.dw, prm.hw, prm.vw)
            assert int(res["score"][a:a + 1].view(np.uint32)[0]) == w["score_bits"] and np.array_equal(paths[a], w["path"]), (prm.subseq, fwd)
        mapped, other = (0, 1) if hit["fwd"] else (1, 0)
        print("example read", "RSUB" if prm.subseq == 1 else "QSUB", "mapped strand", res["score"][mapped], res["mean_score"][mapped],
              "other", res["score"][other], res["mean_score"][other])
        assert res["score"][mapped] < res["score"][other] and res["mean_score"][mapped] < res["mean_score"][other]
    # ref_kmers against the reference's own k-mers (the CPU suite checks the same through the emulator build)
    g = np.load(GOLD / "dtw_goldens.npz")
    off = g["kmers_off"]
    for r, (a, b) in enumerate(g["kmer_ranges"]):
        assert np.array_equal(capi.ref_kmers(ix, EX_PREFIX, 0, int(a), int(b), True), g["kmers_fwd"][int(off[r]):int(off[r + 1])])
        assert np.array_equal(capi.ref_kmers(ix, EX_PREFIX, 0, int(a), int(b), False), g["kmers_rev"][int(off[r]):int(off[r + 1])])


def test_argument_errors_leave_the_gpu_untouched(hip_lib):
    from uncalled_amd import capi
    ev, km = np.full(4, 90, np.float32), np.arange(4, dtype=np.uint16)
    for evs, kms, prm in (([ev[:0]], [km], capi.DTW_EVENT_GLOB), ([ev], [km[:0]], capi.DTW_EVENT_GLOB),
                          ([ev], [km + 1021], capi.DTW_EVENT_GLOB), ([ev], [km], capi.DTWParams(3, 0, 1, 1, 1)),
                          ([ev], [km], capi.DTWParams(0, 2, 1, 1, 1))):
        with pytest.raises(capi.UncalledHipError, match="error -1"):
            capi.dtw_batch(evs, kms, prm, device=63)      # (no such device: a call that reached the runtime would fail with a HIP error)
    scores, _, _ = capi.dtw_batch([ev], [km], capi.DTW_EVENT_GLOB)      # and the next good call works
    assert np.isfinite(scores[0])


def test_more_alignments_than_wavefronts(hip_lib, checker, means):
    """3 x (16 x CUs) + 17 alignments cycling 256 small cases, in every subseq x cost: the launch has 16 x CUs wavefronts, so each
    goes round the queue loop of k_dtw about three times"""
    import torch
    from uncalled_amd import capi
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = 3 * 16 * cus + 17
    for b in dc.queue_batches(means, n, 256, 200):
        assert len(b["evs"]) == n > 16 * cus
        dc.check(checker, b)
        ms, rounds, _ = capi.dtw_last_timing()
        print(f"{b['name']}: {n} alignments on {16 * cus} wavefronts, kernel {ms:.2f} ms, {rounds} round(s)")
        assert rounds == 1


def test_row_and_column_indices_past_65536(hip_lib, checker, means):
    from uncalled_amd import capi
    for b in dc.long_index_batches(means):
        want = dc.wanted(checker, b)
        dc.assert_long_indices_used(b, want)
        res, paths = dc.run(b)
        print(f"{b['name']}: kernel {capi.dtw_last_timing()[0]:.2f} ms")
        assert_equal_to_checker(res, paths, want)


def test_more_than_4_gib_of_back_pointers_in_one_round(hip_lib, checker, means):
    """720 alignments near 6000 x 4000 in a workspace of exactly their sum, 4.41 GB: the BYTE quantities of the round planner (`w * 4`
    against the workspace, the bytes held, the size of the allocation) pass 2^32.  DtwJob::crumb_off counts 32-bit words and stays
    near 1.1e9 here: its width is NOT held by this or any test (a round of about 2880 such alignments, 17.7 GB, would)."""
    from uncalled_amd import capi
    b = dc.big_round_batch(means)
    assert len(b["evs"]) == 720 and b["workspace"] > 2**32
    want = dc.wanted(checker, b)
    res, paths = dc.run(b, workspace_bytes=b["workspace"])
    ms, rounds, held = capi.dtw_last_timing()
    print(f"big round: {len(b['evs'])} alignments, kernel {ms:.2f} ms, {rounds} round(s), {held} bytes of back-pointers held")
    assert rounds == 1 and held == b["workspace"] and held > 2**32
    assert_equal_to_checker(res, paths, want)


def test_offsets_as_a_caller_may_give_them(hip_lib, checker, means):
    from uncalled_amd import capi
    dc.check_caller_offsets(capi.load(), checker, means)
    dc.check_no_paths_with_a_too_large_member(checker, means)


def test_ties_at_the_end_cell(hip_lib, checker, means):
    for b in dc.end_tie_batches(means):
        res, paths, want = dc.check(checker, b)
        dc.assert_end_ties(b, want)
        assert [tuple(int(x) for x in p[0]) for p in paths] == b["end"], b["name"]


def test_ties_in_every_cell_and_events_that_are_no_numbers(hip_lib, checker, means):
    for b in dc.zero_weight_batches(means, 1000, 900):
        _, _, want = dc.check(checker, b)
        assert want[0]["ties"] > 0.99 * 1000 * 900, b["name"]
    for b in dc.rounded_batches(means, 1000, 900, 1.0):
        _, _, want = dc.check(checker, b)
        assert want[0]["ties"] >= 0.01 * 1000 * 900, b["name"]
    for rows, cols in ((200, 200), (150, 130)):
        for b in dc.nonfinite_batches(means, rows, cols):
            dc.check(checker, b)
    b = dc.nan_before_the_end_batch(means)
    _, paths, want = dc.check(checker, b)
    assert want[0]["score"] == 0.0 and want[0]["end_min_cells"] == 1 and not want[0]["last_is_min"]
    assert tuple(int(x) for x in paths[0][0]) == b["end"][0]


def test_two_threads_each_on_a_stream_of_its_own(hip_lib, mixed, mixed_want):
    """unc_dtw_batch from two threads at once: one held to the largest alignment's workspace (3 rounds or more), one free (1 round).
    Each gets the checker's results, and unc_dtw_last_timing tells each thread of its own call.  What this holds is the
    thread_local timing and the buffers of each call; the model's first upload behind its mutex is NOT raced, since the tests
    above have uploaded it long before."""
    import threading
    import torch
    from uncalled_amd import capi
    evs, kms = mixed
    biggest = max(crumb_bytes(k.size, e.size) for e, k in zip(evs, kms))
    prm = capi.DTWParams(1, 1, *WEIGHTS[1])
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    barrier = threading.Barrier(2, timeout=60)
    out = [None, None]

    def work(t, ws):
        try:
            barrier.wait()
            res, paths = capi.dtw_batch(evs, kms, prm, workspace_bytes=ws, stream=streams[t].cuda_stream, full=True)
            out[t] = (res, paths, capi.dtw_last_timing())
        except BaseException as e:      # (reported by the asserts below)
            out[t] = e

    total = sum(crumb_bytes(k.size, e.size) for e, k in zip(evs, kms))
    threads = [threading.Thread(target=work, args=(0, biggest)), threading.Thread(target=work, args=(1, 0))]
    for th in threads:
        th.start()
    for th in threads:
        th.join(300)
        assert not th.is_alive()
    for t in (0, 1):
        assert isinstance(out[t], tuple), out[t]
        assert_equal_to_checker(out[t][0], out[t][1], mixed_want[(1, 1)])
    (_, rounds0, held0), (_, rounds1, held1) = out[0][2], out[1][2]
    print(f"two threads: rounds {rounds0} and {rounds1}, bytes held {held0} and {held1}")
    assert rounds0 >= 3 and held0 <= biggest
    assert rounds1 == 1 and held1 == total
