"""`-m gpu`: the pile-up's level histograms and the Kolmogorov-Smirnov kernel (k_pileup_hist.hip, unc_pileup_hist.cpp) on the MI355X: the
cases of tests/pileup_hist_cases.py that tests/test_pileup_hist_cpu.py runs under the emulator, then `pileup --ks`.

Every test runs inside this one pytest process.  The command-line test starts three children, one after another, each finished before
the next begins."""
import subprocess
import sys

import pytest

import pileup_cases as pc
import pileup_hist_cases as hc
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
    prefix, seqs = rc.multi_reference(tmp_path_factory.mktemp("multi_hist"))
    ctx = pc.Ctx(L, prefix, seqs)
    assert ctx.lens == list(rc.MULTI_LENS) == [len(s) for s in seqs]
    return ctx


def test_layout_and_symbols(L):
    import __graft_entry__ as g
    hc.case_layout(L)
    assert "k_pileup_hist.hip" in g.HIP_INCLUDED


def test_centres(X):
    hc.case_centres(X)


def test_centres_sequences(M):
    hc.case_centres_sequences(M)


def test_bucket_edges(X):
    hc.case_bucket_edges(X)


def test_one_bin_many_workgroups(X):
    hc.case_one_bin(X)


def test_order_split_reset(X):
    pu = hc.case_order_split_reset(X)
    assert pu.last_timing() > 0


def test_merge(X):
    hc.case_merge(X)


def test_enable_refusals(X):
    hc.case_enable_refusals(X)


def test_through_the_alignment(X, reads):
    hc.case_through_the_alignment(X, reads)


def test_ks(X):
    hc.case_ks(X, on_gpu=True)


def test_ks_wide_and_refusals(X):
    hc.case_ks_wide_and_refusals(X)


# ---- the command line
def _cli(*args):
    return subprocess.run([sys.executable, "-m", "uncalled_amd", *[str(a) for a in args]], cwd=str(ROOT), capture_output=True, text=True, timeout=120)


def test_cli_pileup_ks(L, tmp_path):
    """9. the example is ONE read, so the same read is sample and control under --min-cov 1 --ks: every line ends in ks_d 0, ks 0 and
    bucket 0, and its other columns are those of the run without --ks; --ks without --control is an argument error.  Three children"""
    from uncalled_amd import __main__ as cli
    from uncalled_amd import _uncalled_amd as unc
    c = unc.Conf()
    c.bwa_prefix = str(EX_PREFIX)
    pool = unc.MapPool(c)
    pool.add_fast5(str(GOLD / "example_read.fast5"))
    out = []
    while pool.running():
        out += pool.update()
    pool.stop()
    assert len(out) == 1
    (tmp_path / "ex.paf").write_text(str(out[0]) + "\n")
    common = (EX_PREFIX, GOLD / "example_read.fast5", tmp_path / "ex.paf", "--band", "24", "--max-events", "2000", "--region",
              "Escherichia_coli_chromosome:2400000-2410000:6000-7500")
    control = ("--control", GOLD / "example_read.fast5", tmp_path / "ex.paf", "--min-cov", "1")
    r = _cli("pileup", *common, "-o", tmp_path / "two.tsv", *control)
    assert r.returncode == 0, r.stderr
    r = _cli("pileup", *common, "-o", tmp_path / "ks.tsv", *control, "--ks")
    assert r.returncode == 0, r.stderr
    r = _cli("pileup", *common, "-o", tmp_path / "bad.tsv", "--ks")
    assert r.returncode != 0 and "--control" in r.stderr and not (tmp_path / "bad.tsv").exists()
    two = (tmp_path / "two.tsv").read_text().split("\n")
    ks = (tmp_path / "ks.tsv").read_text().split("\n")
    assert len(two) == len(ks) > 22 and two[-1] == ks[-1] == ""
    assert two[0] == "\t".join(cli.PILEUP_COLUMNS + cli.PILEUP_CONTROL_COLUMNS)
    assert ks[0] == two[0] + "\t" + "\t".join(cli.PILEUP_KS_COLUMNS) and cli.PILEUP_KS_COLUMNS == ("ks_d", "ks", "ks_bucket")
    assert [x for x in ks[1:-1]] == [x + "\t0\t0\t0" for x in two[1:-1]]
