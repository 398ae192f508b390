"""GPU: unc_align_batch on the MI355X -- the committed reference results (tests/golden/align_goldens.npz), and, for shapes the
goldens do not hold, the checker chain: the event detector's restatement on the calibrated slice, tests/align_check.c, then
tests/dtw_check.c (tests/align_check.py: expected()).  Every comparison is in bits."""
import numpy as np
import pytest

import align_cases as ac
from conftest import EX_PREFIX, GOLD

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def G():
    return ac.Goldens()


@pytest.fixture(scope="module")
def chain(oracle_lib):
    from align_check import AlignChecker, expected
    from dtw_check import Checker
    a, d = AlignChecker(), Checker()

    def run(signal, cal, query, kmers, **kw):
        return expected(oracle_lib, a, d, signal, cal, query, kmers, **kw)
    return run


def assert_equal_to_chain(r, lev, path, want, tag):
    from uncalled_amd import capi
    assert int(r["n_events"]) == want["n_events"], (tag, "events detected")
    assert int(r["n_kept"]) == want["levels"].size, (tag, "events kept")
    assert np.array_equal(ac.bits([r["tgt_mean"], r["tgt_stdv"]]), ac.bits([want["tgt_mean"], want["tgt_stdv"]])), (tag, "target")
    if want["levels"].size == 0:
        assert int(r["status"]) == capi.ALIGN_NO_COLUMNS, tag
        return
    assert np.array_equal(ac.bits([r["scale"], r["shift"]]), ac.bits([want["scale"], want["shift"]])), (tag, "scale, shift")
    if lev is not None:
        assert np.array_equal(ac.bits(lev), ac.bits(want["levels"])), (tag, "levels")
    assert int(r["status"]) == capi.DTW_OK, tag
    assert int(ac.bits(r["dtw"]["score"])[0]) == want["dtw"]["score_bits"], (tag, "score")
    assert int(ac.bits(r["dtw"]["mean_score"])[0]) == int(ac.bits(want["dtw"]["mean"])[0]), (tag, "mean score")
    assert int(r["dtw"]["path_len"]) == want["dtw"]["path_len"], (tag, "path length")
    if path is not None:
        assert np.array_equal(path, want["dtw"]["path"]), (tag, "path")


def test_every_golden(hip_lib, G):
    seen = 0
    for members in G.groups():
        res, levs, paths = G.run(members, levels=True, paths=True)
        for c, r, lv, p in zip(members, res, levs, paths):
            G.check(c, r, lv, p)
            seen += 1
    assert seen == G.n


@pytest.fixture(scope="module")
def sim_batch(hip_lib, goldens, chain):
    """200 queries over 40 simulated reads of the example index: random slice starts and lengths, both strands -- more queries than
    a wavefront has lanes and no multiple of 64.  The expected results are computed once."""
    from uncalled_amd import capi
    rng = np.random.default_rng(7)
    off = goldens["sim_offsets"][:41].astype(np.uint64)
    raw = goldens["sim_signal"][:int(off[40])]
    ex = np.load(GOLD / "example_read.npz")
    cal = (float(ex["range"]), float(ex["offset"]), float(ex["digitisation"]))
    calib = capi.make_calib(40, *cal)
    ix = capi.Index(EX_PREFIX)
    queries, kms = [], []
    for q in range(200):
        r = int(rng.integers(0, 40))
        n = int(off[r + 1] - off[r])
        ln = int(rng.integers(150, 3000))
        st = int(rng.integers(0, n - ln))
        queries.append((r, st, 0 if q % 17 == 0 else st + ln))
        rst = int(rng.integers(0, 9000))
        kms.append(capi.ref_kmers(ix, EX_PREFIX, 0, rst, rst + int(rng.integers(20, 200)), fwd=bool(q & 1)))
    assert len({st % 8 for _, st, _ in queries}) == 8
    want = [chain(raw[int(off[r]):int(off[r + 1])], cal, (st, en), km) for (r, st, en), km in zip(queries, kms)]
    return dict(raw=raw, off=off, calib=calib, queries=queries, kms=kms, want=want)


def test_200_queries_over_40_simulated_reads_equal_the_checker_chain(hip_lib, sim_batch):
    from uncalled_amd import capi
    b = sim_batch
    res, levs, paths = capi.align_batch(b["raw"], b["off"], b["calib"], b["queries"], b["kms"], levels=True, paths=True)
    assert len(res) == 200 and len(res) % 64 != 0
    for q, (r, lv, p, w) in enumerate(zip(res, levs, paths, b["want"])):
        assert_equal_to_chain(r, lv, p, w, q)
    assert sum(w["levels"].size > 0 for w in b["want"]) > 150


def test_2200_queries_put_several_queries_on_one_wavefront(hip_lib, sim_batch):
    """above 1024 queries k_align_prep carries more than one query per wavefront (launch_align_prep), above 2048 k_events does too:
    the 200 queries eleven times over, each copy equal to the checker chain"""
    from uncalled_amd import capi
    b = sim_batch
    res, levs = capi.align_batch(b["raw"], b["off"], b["calib"], b["queries"] * 11, b["kms"] * 11, levels=True)
    assert len(res) == 2200
    for q, (r, lv) in enumerate(zip(res, levs)):
        assert_equal_to_chain(r, lv, None, b["want"][q % 200], q)


def test_host_samples_and_device_samples_give_the_same(hip_lib, sim_batch):
    import torch
    from uncalled_amd import capi
    b = sim_batch
    dev = torch.from_numpy(np.ascontiguousarray(b["raw"])).cuda()
    torch.cuda.synchronize()
    res = capi.align_batch(dev.data_ptr(), b["off"], b["calib"], b["queries"], b["kms"], on_device=True)
    for q, (r, w) in enumerate(zip(res, b["want"])):
        assert_equal_to_chain(r, None, None, w, q)


def test_a_small_workspace_runs_in_two_rounds_with_the_same_results(hip_lib, sim_batch):
    from uncalled_amd import capi
    b = sim_batch
    one, p1 = capi.align_batch(b["raw"], b["off"], b["calib"], b["queries"], b["kms"], paths=True)
    assert capi.dtw_last_timing()[1] == 1
    total = capi.dtw_last_timing()[2]
    two, p2 = capi.align_batch(b["raw"], b["off"], b["calib"], b["queries"], b["kms"], paths=True, workspace_bytes=int(total * 0.6))
    assert capi.dtw_last_timing()[1] == 2
    assert one.tobytes() == two.tobytes()
    assert all((x is None and y is None) or np.array_equal(x, y) for x, y in zip(p1, p2))


def test_a_large_query_beside_one_event_queries(hip_lib, G, chain):
    """the whole example read (about 6 000 events) against 3 000 k-mers, with 1-event queries before and after it in the batch"""
    from uncalled_amd import capi
    ix = capi.Index(EX_PREFIX)
    one = G.idx("events_1")
    big_km = capi.ref_kmers(ix, EX_PREFIX, 0, 1000, 4004, fwd=False)
    assert big_km.size == 3000
    queries = [G.query(one), (3, 0, 0), G.query(one)]
    kms = [G.kmers(one), big_km, G.kmers(one)]
    res, levs, paths = capi.align_batch(G.raw, G.offsets, G.calib, queries, kms, levels=True, paths=True)
    for i in (0, 2):
        G.check(one, res[i], levs[i], paths[i])
    cal = tuple(float(G.calib[3][f]) for f in ("range", "offset", "digitisation"))
    want = chain(G.signals[3], cal, (0, 0), big_km)
    assert 5000 < want["levels"].size < 7000
    assert_equal_to_chain(res[1], levs[1], paths[1], want, "large")


def test_the_cli_on_the_example_fast5(hip_lib, G, tmp_path, capsys):
    """`python -m uncalled_amd dtw` with two query lines, + and -: as in the reference a later line for the same read replaces the
    earlier one, so each order is run; the printed mean score and the path file equal capi.align_batch on the same inputs"""
    from uncalled_amd import capi
    from uncalled_amd.__main__ import kmer_str, main
    ex = np.load(GOLD / "example_read.npz")
    rid = str(ex["read_id"])
    ix = capi.Index(EX_PREFIX)
    name = ix.seq_names()[0]
    lines = {"+": "%s 10001 14001 %s 6700 7000 +" % (rid, name), "-": "%s 10001 14001 %s 6700 7000 -" % (rid, name)}
    means = capi.dtw_model_tables()[0]
    for last in "+-":
        first = "-" if last == "+" else "+"
        qf = tmp_path / ("q%s.txt" % last)
        qf.write_text(lines[first] + "\n" + lines[last] + "\n")
        prefix = str(tmp_path / ("out%s_" % ("p" if last == "+" else "m")))
        main(["dtw", str(EX_PREFIX), str(GOLD / "example_read.fast5"), str(qf), "-o", prefix])
        out = capsys.readouterr().out.strip().split("\n")
        assert len(out) == 1
        got_id, got_mean, _ = out[0].split("\t")
        km = capi.ref_kmers(ix, EX_PREFIX, 0, 6700, 7000, fwd=last == "+")
        res, levs, paths = capi.align_batch(G.raw, G.offsets, G.calib, [(3, 10001, 14001)], [km], levels=True, paths=True,
                                            opts=capi.align_opts(max_events=50000))
        assert got_id == rid and got_mean == "%.6g" % float(res[0]["dtw"]["mean_score"])
        if last == "-":
            G.check(G.idx("example_slice_rev"), res[0], levs[0], paths[0])
        rows = [ln.split("\t") for ln in open(prefix + rid + ".txt").read().strip().split("\n")]
        assert len(rows) == int(res[0]["dtw"]["path_len"])
        assert [(int(r[0]), int(r[1])) for r in rows] == [tuple(map(int, p)) for p in paths[0][::-1]]
        assert rows[0][:2] == ["0", "0"] and (int(rows[-1][0]), int(rows[-1][1])) == (levs[0].size - 1, km.size - 1)
        for r in rows[:: max(1, len(rows) // 50)]:
            j, i = int(r[0]), int(r[1])
            assert r[2] == kmer_str(km[i]) and r[3] == "%.6g" % levs[0][j] and r[4] == "%.6g" % abs(float(levs[0][j]) - float(means[km[i]]))
