"""CPU: alignments in sample coordinates below the GPU -- k_events.hip's whole-event variant, k_align_prep's col_evt, k_segments.hip
and the host code of unc_align_segments_batch / unc_align_ref_segments_batch under the lanesim emulator, against the checker chain of
tests/segments_cases.py (oracle events -> align_check.c mask -> dtw_check.c path -> segments_check.c).  The cases are those of
tests/test_gpu_segments.py.

The emulator library is the one tests/lanesim/Makefile.align builds.  That make file does not know the sources its sources include
(k_segments.hip, k_refseq.hip, unc_refseq.cpp), and capi.load() keeps one handle per path for the life of the process, so another
test file of the same run may have opened an older build under that path already.  The fixture below rebuilds the library when
it is older than an included source and then loads a COPY of the file as it now is, under a path of its own: the handle these
tests use is the fresh build, whatever was loaded before."""
import shutil
import subprocess

import numpy as np
import pytest

import align_cases as ac
import segments_cases as sc
from conftest import EX_PREFIX, GOLD, ROOT, build_lock

SIM_DIR = ROOT / "tests" / "lanesim"
SIM_LIB = SIM_DIR / "_build_align" / "libuncalled_sim_align.so"


@pytest.fixture(scope="module")
def sim_align_path(tmp_path_factory):
    """a private copy of the emulator library, made after it was brought up to date with every source, included ones too"""
    import __graft_entry__ as g
    mine = tmp_path_factory.mktemp("sim_align") / SIM_LIB.name
    with build_lock():
        sources = [g.CSRC / f for f in g.HIP_INCLUDED + g.HIP_SOURCES] + list(g.CSRC.glob("*.h"))
        stale = SIM_LIB.exists() and any(f.stat().st_mtime > SIM_LIB.stat().st_mtime for f in sources)
        subprocess.run(["make", "-s", "-C", str(SIM_DIR), "-f", "Makefile.align"] + (["-B"] if stale else []), check=True)
        assert all(f.stat().st_mtime <= SIM_LIB.stat().st_mtime for f in sources), "the emulator library is older than a source"
        shutil.copy2(SIM_LIB, mine)
    return mine


@pytest.fixture(scope="module")
def sim_align_lib(sim_align_path):
    from uncalled_amd import capi
    assert str(sim_align_path) not in capi._libs         # nobody can have opened this path before
    L = capi.load(sim_align_path)
    assert hasattr(L, "unc_align_segments_batch") and hasattr(L, "unc_align_ref_segments_batch")
    return L


@pytest.fixture(scope="module")
def chain(oracle_lib):
    return sc.Chain(oracle_lib)


@pytest.fixture(scope="module")
def reads():
    return sc.Reads()


def test_included_kernel_source_is_part_of_the_build():
    import __graft_entry__ as g
    assert "k_segments.hip" in g.HIP_INCLUDED and (g.CSRC / "k_segments.hip").exists()
    assert '#include "k_segments.hip"' in (g.CSRC / "k_align.hip").read_text()


def test_record_layouts():
    from uncalled_amd import capi
    import ctypes
    assert capi.SEGMENT.itemsize == 40 and capi.EVENT.itemsize == 16 and capi.SEG_INFO.itemsize == 16
    assert ctypes.sizeof(capi.AlignSegments) == 40
    assert [capi.SEGMENT.fields[f][1] for f in ("smp_st", "smp_span", "smp_n", "col_first", "n_cols", "mean", "stdv", "level", "shared")] == \
        [0, 8, 12, 16, 20, 24, 28, 32, 36]


def test_checker_on_a_path_by_hand():
    """segments_check.c on a path and events small enough to do by hand: rows 1..2 of three, a vertical move onto row 2, a masked
    event between the columns of row 1"""
    from uncalled_amd import capi
    ev = np.zeros(4, capi.EVENT)
    ev["mean"], ev["stdv"], ev["start"], ev["length"] = [80, 90, 100, 120], [1, 2, 3, 4], [0, 10, 14, 30], [10, 4, 16, 6]
    col_evt = [0, 2, 3]                      # event 1 was masked
    path = np.array([[2, 2], [2, 1], [1, 1], [0, 1]], np.uint32)      # end cell first
    segs, row_first = sc.SegChecker().segments(path, ev, col_evt, 1000, 2.0, -50.0)
    assert row_first == 1 and segs.size == 2
    a, b = segs
    assert (int(a["smp_st"]), int(a["smp_span"]), int(a["smp_n"]), int(a["col_first"]), int(a["n_cols"]), int(a["shared"])) == (1000, 36, 32, 0, 3, 0)
    S, N = 80 * 10 + 100 * 16 + 120 * 6, 32
    Q = 10 * (1 + 6400) + 16 * (9 + 10000) + 6 * (16 + 14400)
    assert a["mean"] == np.float32(S / N) and a["stdv"] == np.float32(np.sqrt(Q / N - (S / N) ** 2))
    assert a["level"] == np.float32(np.float32(2.0) * a["mean"]) + np.float32(-50.0)
    assert (int(b["smp_st"]), int(b["smp_span"]), int(b["smp_n"]), int(b["col_first"]), int(b["n_cols"]), int(b["shared"])) == (1030, 6, 6, 2, 1, 1)
    assert b["mean"] == np.float32(120) and b["stdv"] == np.float32(4)


def test_oracle_events_equal_live_reference_in_every_field(oracle_lib, ref_lib, example, reads):
    """tests/test_oracle.py compares the restatement's events with the reference's own EventDetector by their means; the chain here
    leans on stdv, start and length as well.  The harness under oracle/_ref gives all four: the made reads, slices of them at every
    start modulo 8, and a slice of the example read"""
    po, pr = oracle_lib, ref_lib
    pr.init(example["prefix"])
    sigs = [po.calibrate(s, *sc.CALIB) for s in reads.signals]
    sigs += [sigs[1][st:st + 900] for st in range(200, 208)]
    sigs.append(po.calibrate(example["signal"][10001:14001], example["range"], example["offset"], example["digitisation"]))
    for i, sig in enumerate(sigs):
        ev, rev = po.detect_events(sig)[0], pr.events(sig)[0]
        assert len(ev) == len(rev) > 0, i
        for f in ("mean", "stdv", "start", "length"):
            assert ev[f].tobytes() == rev[f].tobytes(), (i, f)
    assert any((po.detect_events(s)[0]["stdv"] > 0).all() for s in sigs)


@pytest.mark.lanesim
@pytest.mark.parametrize("name", list(sc.CASES))
def test_case_under_the_emulator(name, chain, sim_align_lib, reads):
    sc.CASES[name](chain, sim_align_lib, reads)


@pytest.mark.lanesim
def test_goldens_unchanged_through_the_new_entry_point(sim_align_lib):
    G = ac.Goldens()
    small = [c for c in range(G.n) if G.signals[G.query(c)[0]].size < 20000]
    G.groups = lambda: [[c for c in m if c in small] for m in ac.Goldens.groups(G) if any(c in small for c in m)]
    assert sc.check_goldens_unchanged(G, sim_align_lib) == len(small)


@pytest.fixture(scope="module")
def example_segments(chain, sim_align_lib):
    from uncalled_amd import capi
    G = ac.Goldens()
    ix = capi.Index(EX_PREFIX, lib=sim_align_lib)
    rs = capi.RefSeq(ix, EX_PREFIX)
    segs, kms = sc.check_example(chain, G, rs, ix, str(EX_PREFIX))
    rs.close()
    return segs, kms


@pytest.mark.lanesim
def test_example_read_by_coordinates_and_by_kmers(example_segments):
    segs, kms = example_segments
    assert segs[0].size == kms[0].size == 296 and segs[1].size == 296


@pytest.mark.lanesim
def test_binding_order_by_coordinates_and_by_kmers(sim_align_lib):
    from uncalled_amd import capi
    ix = capi.Index(EX_PREFIX, lib=sim_align_lib)
    rs = capi.RefSeq(ix, EX_PREFIX)
    sc.check_binding_order(ac.Goldens(), rs, ix, str(EX_PREFIX))
    rs.close()


@pytest.mark.lanesim
def test_argument_errors_by_coordinates(sim_align_lib):
    from uncalled_amd import capi
    G = ac.Goldens()
    ix = capi.Index(EX_PREFIX, lib=sim_align_lib)
    rs = capi.RefSeq(ix, EX_PREFIX)
    sc.check_ref_argument_errors(G, rs)
    rs.close()


@pytest.mark.lanesim
def test_binding_returns_what_the_abi_wrote(chain, sim_align_lib, reads):
    from uncalled_amd import capi
    qs, kms = [(0, 0, 800), (0, 100, 100), (0, 900, 1500)], [reads.walk[:80], reads.walk[:5], reads.walk[90:150]]
    res, lev, paths, segs, info, evs = capi.align_batch(reads.raw, reads.offsets, reads.calib, qs, kms, levels=True, paths=True, segments=True,
                                                        events=True, lib=sim_align_lib)
    a = sc.call(sim_align_lib, reads, qs, kms)
    assert res.tobytes() == a["res"].tobytes() and info.tobytes() == a["info"].tobytes()
    assert all(sc.rec_equal(x, y) for x, y in zip(segs, a["segs"])) and all(sc.rec_equal(x, y) for x, y in zip(evs, a["events"]))
    assert segs[1].size == 0 and int(info["status"][1]) == capi.SEG_NONE and paths[1] is None
    only = capi.align_batch(reads.raw, reads.offsets, reads.calib, qs, kms, segments=True, lib=sim_align_lib)
    assert len(only) == 3 and all(sc.rec_equal(x, y) for x, y in zip(only[1], segs))
    assert capi.align_segments_last_timing(sim_align_lib) >= 0


def test_rows_of_the_minus_strand_map_to_forward_positions():
    """segment_ref_pos, the ref_pos of the CLI's table, against the FASTA string: row r of a minus-strand query is the reverse
    complement of the forward k-mer at ref_pos (refalign_cases.py_kmers restates BwaIndex::get_kmers from the string)"""
    from refalign_cases import py_kmers
    from uncalled_amd.__main__ import kmer_str, segment_ref_pos
    rng = np.random.default_rng(3)
    seq = "".join("ACGT"[b] for b in rng.integers(0, 4, 120))
    comp = str.maketrans("ACGT", "TGCA")
    for st, en in ((0, 5), (3, 40), (17, 120)):
        for fwd in (True, False):
            km = py_kmers(seq, st, en, fwd)
            for row in range(km.size):
                pos = segment_ref_pos(st, en, fwd, row)
                fw = seq[pos:pos + 5]
                assert st <= pos <= en - 5 and kmer_str(km[row]) == (fw if fwd else fw[::-1].translate(comp)), (st, en, fwd, row)


@pytest.mark.lanesim
def test_the_cli_writes_the_segments(example_segments, sim_align_lib, sim_align_path, tmp_path, capsys, monkeypatch):
    """`dtw --paf -o P --segments` on the example fixture: one line per record, the capi records' numbers, ref_pos and k-mer checked
    against the FASTA on both strands"""
    from uncalled_amd import capi
    from uncalled_amd.__main__ import main, segment_ref_pos
    monkeypatch.setattr(capi, "DEFAULT_LIB", sim_align_path)
    segs, kms = example_segments
    rid = str(np.load(GOLD / "example_read.npz")["read_id"])
    name = capi.Index(EX_PREFIX, lib=sim_align_lib).seq_names()[0]
    fasta = "".join(ln.strip() for ln in open(str(EX_PREFIX) + ".fa") if not ln.startswith(">"))
    comp = str.maketrans("ACGT", "TGCA")
    means = capi.dtw_model_tables()[0]
    for strand, want, km in (("+", segs[0], kms[0]), ("-", segs[1], kms[1])):
        # PAF read coordinates are bases at 450 / 4000 a sample: the slice [10001, 14001) is not a whole number of bases, so the query file
        # of the path test is used for the samples and the PAF for the rest
        qf = tmp_path / ("q%s.txt" % strand)
        qf.write_text("%s 10001 14001 %s 6700 7000 %s\n" % (rid, name, strand))
        main(["dtw", str(EX_PREFIX), str(GOLD / "example_read.fast5"), str(qf), "-o", str(tmp_path / "s_"), "--segments"])
        capsys.readouterr()
        lines = (tmp_path / ("s_%s.segments.tsv" % rid)).read_text().strip().split("\n")
        assert lines[0].split("\t") == ["ref_name", "ref_pos", "strand", "kmer", "smp_st", "smp_span", "smp_n", "n_cols", "shared", "mean", "stdv",
                                        "level", "model_mean"]
        rows = [ln.split("\t") for ln in lines[1:]]
        assert len(rows) == want.size
        for r, (f, s) in enumerate(zip(rows, want)):
            pos = int(f[1])
            fw = fasta[pos:pos + 5]
            assert f[0] == name and f[2] == strand and f[3] == (fw if strand == "+" else fw[::-1].translate(comp)), (r, f)
            assert pos == segment_ref_pos(6700, 7000, strand == "+", r)
            assert [int(x) for x in f[4:9]] == [int(s[k]) for k in ("smp_st", "smp_span", "smp_n", "n_cols", "shared")], (r, f)
            assert f[9:12] == ["%.6g" % float(s[k]) for k in ("mean", "stdv", "level")] and f[12] == "%.6g" % float(means[km[r]]), (r, f)
    # PAF input: the same file through --paf (the sample range then comes from the PAF's base coordinates)
    paf = tmp_path / "q.paf"
    paf.write_text("\t".join([rid, "3563", "1125", "1575", "-", name, "10000", "6700", "7000", "100", "300", "60"]) + "\n")
    main(["dtw", str(EX_PREFIX), str(GOLD / "example_read.fast5"), str(paf), "--paf", "-o", str(tmp_path / "p_"), "--segments"])
    capsys.readouterr()
    lines = (tmp_path / ("p_%s.segments.tsv" % rid)).read_text().strip().split("\n")
    assert len(lines) == 297 and int(lines[1].split("\t")[4]) >= 10000 and lines[1].split("\t")[1] == "6995"
    with pytest.raises(SystemExit):
        main(["dtw", str(EX_PREFIX), str(GOLD / "example_read.fast5"), str(paf), "--paf", "--segments"])       # needs -o
