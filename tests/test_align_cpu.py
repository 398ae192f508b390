"""CPU: read-to-reference alignment below the GPU -- the checker (tests/align_check.c) against the committed reference results
(tests/golden/align_goldens.npz, written by tests/golden/make_align_goldens.py), and k_align.hip, k_events.hip, k_dtw.hip and
unc_align.cpp themselves under the lanesim emulator (built by tests/lanesim/Makefile.align, a make file of its own).

Each stage's test was seen to fail once under the emulator with a defect put in by hand and taken out again
(test_kernels_under_the_emulator_equal_every_golden, and with it the two tests that run goldens in other batches):
  * the slice's first sample rounded down to a multiple of 8 in unc_align.cpp: ('start_mod8_1', 'scale') -- the slice had its
    events by count and not by value -- and "49 == 50" events kept for events_50 in the test of the statuses;
  * the tail loop of stall_mask dropped (the events still undecided at the end kept): ('stalls', 'events kept', 420, 396);
  * the target's running sum kept in double and rounded once: ('whole_read', 'tgt_mean'), ('events_26', 'tgt_mean').
For the argument errors and the statuses no defect was put in: they are host code whose tests name the expected outcome directly.
Measured on the build container, one process: the whole file 4 s once the emulator library is built (90 s with its build)."""
import ctypes

import numpy as np
import pytest

import align_cases as ac
from conftest import ROOT, locked_make


@pytest.fixture(scope="module")
def G():
    return ac.Goldens()


@pytest.fixture(scope="module")
def sim_align_lib():
    from uncalled_amd import capi
    locked_make("-C", str(ROOT / "tests" / "lanesim"), "-f", "Makefile.align")
    return capi.load(ROOT / "tests" / "lanesim" / "_build_align" / "libuncalled_sim_align.so")


def test_goldens_cover_what_they_should(G):
    from uncalled_amd import capi
    g = G.g
    st = {n: int(g["smp_st"][G.idx(n)]) for n in G.names}
    assert {st["start_mod8_%d" % r] % 8 for r in range(8)} == set(range(8))
    c = G.idx("to_the_end")
    assert g["smp_en"][c] == 0 and g["smp_st"][c] != 0
    assert any(g["smp_st"][c] == 0 and g["smp_en"][c] == 0 for c in range(G.n))
    assert np.bincount(g["sig"]).max() >= 2           # several queries on one read
    n_ev = {n: int(g["ev_off"][G.idx(n) + 1] - g["ev_off"][G.idx(n)]) for n in G.names}
    for want in (0, 1, 12, 13, 24, 25, 26, 50):
        assert n_ev["events_%d" % want] == want
    assert 200 <= n_ev["few_hundred"] <= 500
    m = G.seg("mask", "ev_off", G.idx("stalls")).astype(bool)
    runs = np.flatnonzero(np.diff(np.concatenate([[1], m.astype(int), [1]])))
    assert not m[0] and not m[-1] and runs.size == 6 and (~m[-24:]).all()      # stalls at the head, in the middle and at the tail
    assert n_ev["all_masked"] >= 25 and not G.seg("mask", "ev_off", G.idx("all_masked")).any()
    assert g["flags"][G.idx("mask_off")] & capi.ALIGN_NO_MASK and g["flags"][G.idx("raw")] & capi.ALIGN_RAW
    assert g["flags"][G.idx("target_model")] & capi.ALIGN_TARGET_MODEL
    assert G.kmers(G.idx("one_kmer")).size == 1 and g["tgt_bits"][G.idx("one_kmer")][1] == 0 and G.kmers(G.idx("two_kmers")).size == 2
    assert set(map(int, g["cost"])) == {0, 1} and {0, 1} <= set(map(int, g["subseq"]))
    assert sum(int(s) == 3 for s in g["sig"]) >= 2     # the example read, both strands


def test_checker_reproduces_every_golden(G, oracle_lib):
    """tests/align_check.c (stages b to d) between the detector's restatement and tests/dtw_check.c: every stage in bits"""
    from align_check import AlignChecker, expected
    from dtw_check import Checker
    from uncalled_amd import capi
    chk, dchk, g = AlignChecker(), Checker(), G.g
    mt = tuple(g["model_target_bits"].view(np.float32))
    assert np.array_equal(ac.bits(capi.align_model_target()), g["model_target_bits"])
    for c in range(G.n):
        s, st, en = G.query(c)
        fl = int(g["flags"][c])
        cal = tuple(float(G.calib[s][f]) for f in ("range", "offset", "digitisation"))
        r = expected(oracle_lib, chk, dchk, G.signals[s], cal, (st, en), G.kmers(c), mask=not fl & capi.ALIGN_NO_MASK,
                     create_events=not fl & capi.ALIGN_RAW, target="model" if fl & capi.ALIGN_TARGET_MODEL else "kmers", model_target=mt,
                     dtw=(int(g["subseq"][c]), int(g["cost"][c]), *map(float, g["weights"][c])))
        name = G.names[c]
        if not fl & capi.ALIGN_RAW:
            assert r["n_events"] == G.seg("events", "ev_off", c).size, name
            if not fl & capi.ALIGN_NO_MASK:
                assert np.array_equal(r["mask"], G.seg("mask", "ev_off", c).astype(bool)), name
        want_lev = G.seg("levels", "lev_off", c)
        assert np.array_equal(ac.bits(r["levels"]), ac.bits(want_lev)), name
        got = ac.bits([r["tgt_mean"], r["tgt_stdv"], r["scale"], r["shift"]])
        assert np.array_equal(got[:2], g["tgt_bits"][c][:2]) and (want_lev.size == 0 or np.array_equal(got[2:], g["tgt_bits"][c][2:])), name
        if want_lev.size:
            assert r["dtw"]["score_bits"] == int(g["score_bits"][c]) and int(ac.bits(r["dtw"]["mean"])[0]) == int(g["mean_bits"][c]), name
            assert np.array_equal(r["dtw"]["path"], g["path"][2 * int(g["path_off"][c]):2 * int(g["path_off"][c + 1])].reshape(-1, 2)), name


def test_library_exports_the_align_entry_points():
    import __graft_entry__ as g
    assert "k_align.hip" in g.HIP_SOURCES and "unc_align.cpp" in g.HIP_SOURCES
    L = ctypes.CDLL(str(g.build_hip()))      # hipcc cross-compiles for gfx950 without a GPU
    for s in ("unc_align_batch", "unc_align_last_timing", "unc_align_model_target"):
        assert hasattr(L, s), s
    from uncalled_amd import capi
    assert capi.ALIGN_RESULT.itemsize == 56 and capi.ALIGN_QUERY.itemsize == 24 and ctypes.sizeof(capi.AlignOpts) == 32


@pytest.mark.lanesim
def test_kernels_under_the_emulator_equal_every_golden(G, sim_align_lib):
    """every golden through unc_align_batch, the cases that share their options in one batch (mixed reads, slices and sizes share
    the launches): counts, target, scale, shift, levels, score, mean score and path in bits"""
    seen = 0
    for members in G.groups():
        res, levs, paths = G.run(members, lib=sim_align_lib, levels=True, paths=True)
        for c, r, lv, p in zip(members, res, levs, paths):
            G.check(c, r, lv, p)
            seen += 1
    assert seen == G.n


@pytest.mark.lanesim
def test_levels_and_paths_absent_and_the_default_options(G, sim_align_lib):
    """no levels, no paths: the same records; opts = None is dtw_test (events, mask, k-mer target, DTWr94d / NONE / 1, 1, 1)"""
    from uncalled_amd import capi
    members = [c for c in max(G.groups(), key=len) if G.signals[G.query(c)[0]].size < 20000]
    assert (int(G.g["flags"][members[0]]), int(G.g["subseq"][members[0]]), int(G.g["cost"][members[0]])) == (0, 0, 1)
    res = capi.align_batch(G.raw, G.offsets, G.calib, [G.query(c) for c in members], [G.kmers(c) for c in members], lib=sim_align_lib)
    assert isinstance(res, np.ndarray)
    for c, r in zip(members, res):
        G.check(c, r)
    res2, paths = G.run(members, lib=sim_align_lib, paths=True, workspace_bytes=200000)     # several rounds: the same results
    assert capi.dtw_last_timing(sim_align_lib)[1] >= 2
    for c, r, p in zip(members, res2, paths):
        G.check(c, r, None, p)


@pytest.mark.lanesim
def test_the_two_new_statuses_beside_computed_queries(G, sim_align_lib):
    from uncalled_amd import capi
    members = [G.idx(n) for n in ("events_50", "events_0", "events_26", "all_masked", "events_25", "stalls")]
    res, levs, paths = G.run(members, lib=sim_align_lib, levels=True, paths=True, opts=G.opts(members[0], max_events=26))
    st = [int(r["status"]) for r in res]
    assert st == [capi.ALIGN_TOO_MANY, capi.ALIGN_NO_COLUMNS, capi.DTW_OK, capi.ALIGN_NO_COLUMNS, capi.DTW_OK, capi.ALIGN_TOO_MANY]
    for c, r, lv, p in zip(members, res, levs, paths):
        if int(r["status"]) == capi.ALIGN_TOO_MANY:       # counted and normalised, not aligned
            assert int(r["n_kept"]) == G.seg("levels", "lev_off", c).size and p is None and int(r["dtw"]["path_len"]) == 0
            assert np.array_equal(ac.bits(lv), ac.bits(G.seg("levels", "lev_off", c)))
        else:
            G.check(c, r, lv, p)


@pytest.mark.lanesim
def test_argument_errors_under_the_emulator(G, sim_align_lib):
    from uncalled_amd import capi
    km = np.arange(4, dtype=np.uint16)
    n0 = G.signals[0].size

    def call(q, k=km, opts=None):
        return capi.align_batch(G.raw, G.offsets, G.calib, [q], [k], opts=opts, lib=sim_align_lib)
    for q, k, o in (((0, 0, n0 + 1), km, None),             # a slice outside its read
                    ((0, n0 + 1, 0), km, None),
                    ((0, 200, 100), km, None),              # smp_st > smp_en
                    ((0, 0, 100), km[:0], None),            # no k-mers
                    ((len(G.signals), 0, 0), km, None),     # no such read
                    ((0, 0, 100), km + 1021, None),         # a k-mer past the model
                    ((0, 0, 100), km, capi.align_opts(dtw=capi.DTWParams(3, 0, 1, 1, 1))),
                    ((0, 0, 100), km, capi.align_opts(dtw=capi.DTWParams(0, 2, 1, 1, 1)))):
        with pytest.raises(capi.UncalledHipError, match="error -1"):
            call(q, k, o)
    assert int(call((0, n0, 0))[0]["status"]) == capi.ALIGN_NO_COLUMNS      # an empty slice at the read's end is inside the read
    assert int(call((0, 100, 100))[0]["status"]) == capi.ALIGN_NO_COLUMNS


@pytest.mark.lanesim
def test_the_cli_under_the_emulator(G, sim_align_lib, tmp_path, capsys, monkeypatch):
    """`python -m uncalled_amd dtw` in this process with the emulator build in the library's place: the fast5 reader's read filter,
    the query file (a later line for a read replaces the earlier one, as in the reference), the k-mers of the '-' strand, the
    printed line and the path file, against the golden of the same slice and stretch"""
    from uncalled_amd import capi
    from uncalled_amd.__main__ import kmer_str, main
    from conftest import EX_PREFIX, GOLD
    monkeypatch.setattr(capi, "DEFAULT_LIB", ROOT / "tests" / "lanesim" / "_build_align" / "libuncalled_sim_align.so")
    c = G.idx("example_slice_rev")
    rid = str(np.load(GOLD / "example_read.npz")["read_id"])
    name = capi.Index(EX_PREFIX, lib=sim_align_lib).seq_names()[0]
    qf = tmp_path / "q.txt"
    qf.write_text("%s 10001 14001 %s 6700 7000 +\n%s 10001 14001 %s 6700 7000 -\n" % (rid, name, rid, name))
    main(["dtw", str(EX_PREFIX), str(GOLD / "example_read.fast5"), str(qf), "-o", str(tmp_path / "p_")])
    out = capsys.readouterr().out.strip().split("\n")
    assert len(out) == 1
    got_id, got_mean, _ = out[0].split("\t")
    assert got_id == rid and got_mean == "%.6g" % float(G.g["mean_bits"][c:c + 1].view(np.float32)[0])
    rows = [ln.split("\t") for ln in (tmp_path / ("p_%s.txt" % rid)).read_text().strip().split("\n")]
    want = G.g["path"][2 * int(G.g["path_off"][c]):2 * int(G.g["path_off"][c + 1])].reshape(-1, 2)[::-1]
    assert [(int(r[0]), int(r[1])) for r in rows] == [tuple(map(int, p)) for p in want]
    lev, km = G.seg("levels", "lev_off", c), G.kmers(c)
    assert rows[0][:2] == ["0", "0"] and rows[0][2] == kmer_str(km[0]) and rows[0][3] == "%.6g" % lev[0]
    # --max-events below the slice's 774 events: skipped, as dtw_test skips above 50000
    main(["dtw", str(EX_PREFIX), str(GOLD / "example_read.fast5"), str(qf), "--max-events", "700"])
    cap = capsys.readouterr()
    assert cap.out == "" and "Skipping " + rid in cap.err
