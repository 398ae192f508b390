"""`-m gpu`: the pore model object, the training accumulator (k_model.hip) and the model in the alignment and in the mapper on the
MI355X: the cases of tests/model_cases.py that tests/test_model_cpu.py runs under the emulator, then what needs the mapper and the
host module -- Index.set_model, Conf.model_path, `--model` and `train`.

The reference harness under oracle/ has no model setter, so there are no reference-side goldens for a perturbed model in the
mapper; cases 2 (the tables), 17 (a loaded default maps as the built-in) and 18 (match probabilities of a random model by the
checker's formula) stand in for them."""
import subprocess
import sys

import numpy as np
import pytest

import model_cases as mc
import segments_cases as sc
from conftest import EX_PREFIX, GOLD, ROOT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L(hip_lib):
    import torch
    assert torch.cuda.is_available()
    return hip_lib


@pytest.fixture(scope="module")
def reads():
    return sc.Reads()


def test_default_pairs(L):
    mc.case_default_pairs(L)


def test_default_tables_are_the_index_s_and_the_dtw_s(L):
    from uncalled_amd import capi
    mc.case_default_tables(L, capi.Index(EX_PREFIX, lib=L))


def test_save_load_round_trip_and_shuffled_order(L, tmp_path):
    mc.case_round_trip(L, tmp_path)


def test_random_tables_against_model_check(L):
    mc.case_random_tables(L)


def test_acc_one_bin_two_workgroups(L):
    mc.case_one_bin(L)


def test_acc_carry_into_the_high_word(L):
    mc.case_carry(L)


def test_acc_dropped_and_skipped(L):
    mc.case_drop_and_skip(L)


def test_acc_split_and_order(L):
    from uncalled_amd import capi
    acc, _ = mc.case_split_and_order(L)
    assert acc.last_timing() > 0
    ms = capi.C.c_float(-1)
    L.unc_model_acc_last_timing(capi.C.byref(ms))
    assert ms.value > 0


def test_acc_finish(L):
    mc.case_finish(L)


def test_align_accumulates(L, reads):
    mc.case_align_accumulates(L, reads)


def test_align_short_room(L, reads):
    mc.case_align_short_room(L, reads)


def test_default_model_changes_nothing(L, reads):
    mc.case_default_model_changes_nothing(L, reads)


def test_random_model_alignment(L, reads, oracle_lib):
    mc.case_random_model_alignment(L, reads, oracle_lib)


def test_dtw_model_batch(L):
    mc.case_dtw_model_batch(L)


def test_index_set_model(L, example, goldens):
    mc.case_set_model(L, example, goldens)


# ---- the host module and the command line
EXAMPLE_COLS = ("f41a60f7-de4a-4b17-9f54-387e52d60b65\t106\t73\t106\t-\tEscherichia_coli_chromosome:2400000-2410000\t10000\t6938\t6976\t38\t39\t255"
                "\tch:i:486\tst:i:257117\tmt:f:")


def _cli(*args):
    return subprocess.run([sys.executable, "-m", "uncalled_amd", *[str(a) for a in args]], cwd=str(ROOT), capture_output=True, text=True, timeout=120)


def test_map_pool_reads_model_path(L, tmp_path):
    """20. Conf.model_path: the default model written to a file reproduces the example's PAF line (that the index then holds
    the file's model and not the built-in one by another way: test_index_set_model); a missing file fails (through the command line, which checks the file before the pool is made)"""
    from uncalled_amd import _uncalled_amd as unc
    from uncalled_amd import capi
    capi.Model.default(lib=L).save(tmp_path / "r94.txt")
    c = unc.Conf()
    c.bwa_prefix = str(EX_PREFIX)
    c.model_path = str(tmp_path / "r94.txt")
    pool = unc.MapPool(c)
    pool.add_fast5(str(GOLD / "example_read.fast5"))
    out = []
    while pool.running():
        out += pool.update()
    pool.stop()
    assert len(out) == 1 and str(out[0]).startswith(EXAMPLE_COLS)
    r = _cli("map", EX_PREFIX, GOLD / "example_read.fast5", "--model", tmp_path / "none.txt")
    assert r.returncode != 0 and "none.txt" in r.stderr and not r.stdout.strip()


def test_cli_train(L, tmp_path):
    """21. `train` on the example fast5 and the PAF line MapPool (`map`) gives for it, two iterations with a band: the file loads and equals the
    same two iterations driven through capi"""
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
    r = _cli("train", EX_PREFIX, GOLD / "example_read.fast5", tmp_path / "ex.paf", "-o", tmp_path / "trained.txt", "--iters", "2", "--band", "24",
             "--min-obs", "2", "--max-events", "2000", "--keep-shared")
    assert r.returncode == 0, r.stderr
    rows = [ln for ln in r.stderr.split("\n") if ln.startswith("iteration ")]
    assert len(rows) == 2 and "records used" in rows[0]
    got = capi.Model.load(tmp_path / "trained.txt", lib=L)

    queries = cli.load_paf_queries(str(tmp_path / "ex.paf"))
    rd = cli.load_query_reads(unc, str(GOLD / "example_read.fast5"), queries)
    cli.clip_paf_queries(queries, rd)
    assert len(rd) == 1
    rid, raw, cal = rd[0]
    q = queries[rid]
    index = capi.Index(EX_PREFIX, lib=L)
    refseq = capi.RefSeq(index, EX_PREFIX)
    calib = capi.make_calib(1, 0, 0, 1)
    calib[0] = cal
    offsets = np.array([0, len(raw)], np.uint64)
    stretch = [(index.seq_names().index(q["ref"]), q["ref_st"], q["ref_en"], q["fwd"])]
    model = capi.Model.default(lib=L)
    used = []
    for _ in range(2):
        acc = capi.ModelAcc(keep_shared=True, lib=L)
        res = capi.align_ref_batch(refseq, np.asarray(raw, np.int16), offsets, calib, [(0, q["smp_st"], q["smp_en"])], stretch,
                                   opts=capi.align_opts(max_events=2000, band=24), model=model, accumulate=acc)
        assert int(res["status"][0]) == capi.DTW_OK
        used.append(int(acc.read()[0].sum()))
        model, _ = acc.finish(model, 2)
    assert used[0] > 20 and ("iteration 1: %d records used" % used[0]) in rows[0]
    assert got.pairs().tobytes() == model.pairs().tobytes()
