"""`-m gpu`: the signal pile-up (k_pileup.hip, unc_pileup.cpp) on the MI355X: the cases of tests/pileup_cases.py that
tests/test_pileup_cpu.py runs under the emulator, then the `pileup` command."""
import subprocess
import sys

import numpy as np
import pytest

import pileup_cases as pc
import refalign_cases as rc
import segments_cases as sc
from conftest import EX_PREFIX, GOLD, ROOT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L(hip_lib):
    import torch
    assert torch.cuda.is_available()
    return hip_lib


@pytest.fixture(scope="module")
def X(L):
    return pc.Ctx(L, EX_PREFIX)


@pytest.fixture(scope="module")
def reads():
    return sc.Reads()


@pytest.fixture(scope="module")
def M(L, tmp_path_factory):
    """five sequences; the default table must keep k_pileup_scan at three passes"""
    prefix, seqs = rc.multi_reference(tmp_path_factory.mktemp("multi"))
    ctx = pc.Ctx(L, prefix, seqs)
    assert ctx.lens == list(rc.MULTI_LENS) == [len(s) for s in seqs]
    n_bins = ctx.pileup().n_bins()
    assert n_bins == 528106 and -(-n_bins // pc.SCAN_CHUNK) == 516
    return ctx


def test_layout_and_symbols(L):
    pc.case_layout(L)


def test_one_bin_many_workgroups(X):
    pc.case_one_bin(X)


def test_carry_and_sign(X):
    pc.case_carry(X)


def test_dropped_skipped_outside(X):
    pc.case_dropped_skipped_outside(X)


def test_strands(X):
    pc.case_strands(X)


def test_order_and_split(X):
    from uncalled_amd import capi
    pu = pc.case_order_and_split(X)
    assert pu.last_timing() > 0
    ms = capi.C.c_float(-1)
    X.L.unc_pileup_last_timing(capi.C.byref(ms))
    assert ms.value > 0


def test_regions(X):
    pc.case_regions(X)


def test_through_the_alignment(X, reads):
    pc.case_through_the_alignment(X, reads)


def test_with_an_accumulator(X, reads):
    pu = pc.case_with_an_accumulator(X, reads)
    assert pu.last_timing() > 0


def test_covered(X):
    pu = pc.case_covered(X)
    assert all(t > 0 for t in pu.covered_last_timing())


def test_stats_and_compare(X):
    pc.case_stats_and_compare(X)


def test_merge(X):
    pc.case_merge(X)


def test_refusals(X, reads):
    pc.case_refusals(X, reads)


def test_sequences(M):
    pc.case_sequences(M)


def test_stats_sequences(M):
    pc.case_stats_sequences(M)


@pytest.mark.parametrize("fill", ["a", "b", "c", "d", "e"])
def test_scan_passes(M, fill):
    """the only check of the barriers around k_pileup_scan's reuse of its shared words: the emulator runs the lanes in order"""
    pc.case_scan_passes(M, fill, on_gpu=True)


def test_scan_merge_gather(M):
    pc.case_scan_merge_gather(M)


def test_alignment_sequences(M, reads):
    pc.case_alignment_sequences(M, reads)


def test_alignment_sequences_band_and_cut(M, reads):
    pc.case_alignment_sequences_band_and_cut(M, reads)


def test_alignment_sequences_accumulator_and_regions(M, reads):
    pc.case_alignment_sequences_accumulator_and_regions(M, reads)


# ---- the command line
EXAMPLE_COLS = ("f41a60f7-de4a-4b17-9f54-387e52d60b65\t106\t73\t106\t-\tEscherichia_coli_chromosome:2400000-2410000\t10000\t6938\t6976\t38\t39\t255"
                "\tch:i:486\tst:i:257117\tmt:f:")


def _cli(*args):
    return subprocess.run([sys.executable, "-m", "uncalled_amd", *[str(a) for a in args]], cwd=str(ROOT), capture_output=True, text=True, timeout=120)


def test_cli_pileup(L, tmp_path):
    """14. `pileup` on the example fast5 and the PAF line MapPool (`map`) gives for it, alone and with the same files as the control:
    the TSV text equals the lines built here through capi.  The example is ONE read, so every covered bin holds one record: with the
    control being the sample every line's t is nan under --min-cov 1 (Welch's t needs two records a side) and nothing is covered under
    the default of 2; that t is 0 for equal samples of two records and more is case 10's (compare(a, a))."""
    from uncalled_amd import __main__ as cli
    from uncalled_amd import _uncalled_amd as unc
    from uncalled_amd import capi
    c = unc.Conf()
    c.bwa_prefix = str(EX_PREFIX)
    pool = unc.MapPool(c)
    pool.add_fast5(str(GOLD / "example_read.fast5"))
    out = []
    while pool.running():
        out += pool.update()
    pool.stop()
    assert len(out) == 1 and str(out[0]).startswith(EXAMPLE_COLS)
    (tmp_path / "ex.paf").write_text(str(out[0]) + "\n")
    common = (EX_PREFIX, GOLD / "example_read.fast5", tmp_path / "ex.paf", "--band", "24", "--max-events", "2000")
    r = _cli("pileup", *common, "-o", tmp_path / "one.tsv")
    assert r.returncode == 0, r.stderr
    r = _cli("pileup", *common, "-o", tmp_path / "two.tsv", "--control", GOLD / "example_read.fast5", tmp_path / "ex.paf", "--min-cov", "1")
    assert r.returncode == 0, r.stderr
    r = _cli("pileup", *common, "-o", tmp_path / "none.tsv", "--control", GOLD / "example_read.fast5", tmp_path / "ex.paf",
             "--region", "Escherichia_coli_chromosome:2400000-2410000:6000-7500")
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "none.tsv").read_text().split("\n")[1:] == [""]          # one read: no bin holds two records

    queries = cli.load_paf_queries(str(tmp_path / "ex.paf"))
    rd = cli.load_query_reads(unc, str(GOLD / "example_read.fast5"), queries)
    cli.clip_paf_queries(queries, rd)
    rid, raw, cal = rd[0]
    q = queries[rid]
    index = capi.Index(EX_PREFIX, lib=L)
    names = index.seq_names()
    refseq = capi.RefSeq(index, EX_PREFIX)
    calib = capi.make_calib(1, 0, 0, 1)
    calib[0] = cal
    pu = capi.Pileup(refseq, lib=L)
    res = capi.align_ref_batch(refseq, np.asarray(raw, np.int16), np.array([0, len(raw)], np.uint64), calib, [(0, q["smp_st"], q["smp_en"])],
                               [(names.index(q["ref"]), q["ref_st"], q["ref_en"], q["fwd"])], opts=capi.align_opts(max_events=2000, band=24),
                               pileup=pu)
    assert int(res["status"][0]) == capi.DTW_OK and pu.last_timing() > 0
    ms = capi.C.c_float(-1)
    L.unc_pileup_last_timing(capi.C.byref(ms))
    assert ms.value > 0
    bins = pu.covered(1)
    assert 20 < bins.size <= q["ref_en"] - q["ref_st"] - 4 and pu.counters()[2] == bins.size
    rids, pos, fwd = pu.locate(bins)
    st = pu.stats(bins)
    assert not fwd.any() and int(pos.min()) >= q["ref_st"] and int(pos.max()) <= q["ref_en"] - 5
    lines = ["\t".join(cli.PILEUP_COLUMNS)]
    for i in range(bins.size):
        lines.append("%s\t%d\t-\t%s\t%d\t%.17g\t%.17g\t%.17g\t%.17g\t%.17g\t%.17g" % (
            names[int(rids[i])], int(pos[i]), cli.kmer_str(st["kmer"][i]), int(st["n"][i]), st["mean"][i], st["sd"][i], st["dwell"][i],
            st["model_mean"][i], st["model_stdv"][i], st["z"][i]))
    assert (tmp_path / "one.tsv").read_text() == "\n".join(lines) + "\n"
    two = ["\t".join(cli.PILEUP_COLUMNS + cli.PILEUP_CONTROL_COLUMNS)]
    for i in range(bins.size):
        two.append(lines[i + 1] + "\t%d\t%.17g\t%.17g\tnan" % (int(st["n"][i]), st["mean"][i], st["sd"][i]))
    assert (tmp_path / "two.tsv").read_text() == "\n".join(two) + "\n"
