"""GPU: repeat masking on the MI355X -- the cases of tests/mask_cases.py (the same ones tests/test_mask_cpu.py runs under the
emulator) through the gfx950 library, compared for exact equality with tests/mask_naive.py, and `python -m uncalled_amd mask
internal / external` on the bundled example reference and on the tiny reference: file names, FASTA layout, the BED, and the lines
on stderr and stdout against what the checker and the formats of the reference's scripts give."""
import subprocess
import sys

import pytest

import mask_cases as mc
import mask_naive as mn
from conftest import EX_PREFIX, ROOT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tiny(tmp_path_factory):
    return mc.make_tiny(tmp_path_factory.mktemp("mask_tiny_gpu"))


@pytest.mark.parametrize("case", mc.internal_cases(), ids=lambda c: c["name"])
def test_internal_masking(case, hip_lib):
    from uncalled_amd import capi
    mc.check_internal(capi, case, lib=hip_lib)


def test_every_kernel_goes_round_its_grid_stride_loop(tiny, hip_lib, monkeypatch):
    from uncalled_amd import capi
    monkeypatch.setenv("UNC_MASK_BLOCKS", "2")
    mc.check_grid_strides(capi, tiny, lib=hip_lib)


def test_arguments_and_lifecycle(hip_lib):
    from uncalled_amd import capi
    mc.check_arguments(capi, lib=hip_lib)
    mc.check_lifecycle(capi, lib=hip_lib)


@pytest.mark.parametrize("fm32", [True, False], ids=["fm32", "64-bit"])
@pytest.mark.parametrize("min_len", [2, 50, 120])
def test_external_masking_of_the_tiny_reference(min_len, fm32, tiny, hip_lib):
    from uncalled_amd import capi
    ix = mc.load_index(capi, tiny["prefix"], hip_lib, fm32=fm32)
    out = mc.check_external(capi, ix, tiny["text"], tiny["seqs"], min_len, (1, 5), lib=hip_lib, naive_counts=mc.tiny_counts(tiny, min_len))
    assert out[1][2] >= out[5][2] > 0 and (min_len == 2 or out[1][2] > out[5][2])       # (every 2-mer occurs more than five times)
    ix.close()


@pytest.mark.parametrize("fm32", [True, False], ids=["fm32", "64-bit"])
def test_external_masking_of_a_subset_and_across_junctions(fm32, tiny, hip_lib):
    from uncalled_amd import capi
    ix = mc.load_index(capi, tiny["prefix"], hip_lib, fm32=fm32)
    mc.check_external_arguments(capi, ix, lib=hip_lib)
    mc.check_external(capi, ix, tiny["text"], [tiny["seqs"][1][60:700]], 50, (1, 5), lib=hip_lib)
    targets = mc.junction_targets(tiny["text"], tiny["seqs"])
    counts = mn.window_counts(tiny["text"], targets, 50)
    assert counts[0][4] == 1 and counts[1][0] == 1
    mc.check_external(capi, ix, tiny["text"], targets, 50, (1,), lib=hip_lib, naive_counts=counts)
    ix.close()


@pytest.mark.parametrize("fm32", [True, False], ids=["fm32", "64-bit"])
def test_external_masking_of_the_example_reference(fm32, hip_lib):
    from uncalled_amd import build_index, capi
    _, _, seqs = build_index.read_fasta(str(EX_PREFIX) + ".fa")
    ix = mc.load_index(capi, EX_PREFIX, hip_lib, fm32=fm32)
    out = mc.check_external(capi, ix, mn.pac_text(EX_PREFIX), seqs, 50, (1,), lib=hip_lib)
    assert out[1][2] == 0 and out[1][0] == seqs
    ix.close()


def run_cli(*args):
    return subprocess.run([sys.executable, "-m", "uncalled_amd", "mask", *map(str, args)], cwd=str(ROOT), capture_output=True, text=True)


def iteration_lines(stderr):
    """the lines the subcommand writes to stderr (whatever the runtime adds to them on a given machine aside)"""
    return "".join(l + "\n" for l in stderr.splitlines() if l.startswith("Iteration "))


def fasta_records(path):
    lines = path.read_text().split("\n")
    assert lines[-1] == "" and len(lines) % 2 == 1
    return lines[0:-1:2], lines[1:-1:2]


def test_cli_internal_on_the_example_reference(tmp_path):
    from uncalled_amd import build_index
    fa = str(EX_PREFIX) + ".fa"
    names, annos, seqs = build_index.read_fasta(fa)
    k, iters = 6, 4
    want_seqs, want_report = mn.mask_internal(seqs, k, iters)
    assert len(want_report) == iters
    r = run_cli("internal", fa, k, iters, str(tmp_path) + "/ex_")
    assert r.returncode == 0, r.stderr
    assert iteration_lines(r.stderr) == "".join("Iteration %d: masked %d occurences of %s\n" % (i, occ, kmer) for i, (kmer, occ, _) in enumerate(want_report))
    assert sorted(p.name for p in tmp_path.iterdir()) == ["ex_mask%d.fa" % iters]
    hdrs, got = fasta_records(tmp_path / ("ex_mask%d.fa" % iters))
    assert hdrs == [">" + n + (" " + a if a else "") for n, a in zip(names, annos)] and got == want_seqs
    # the early stop names the file by the iterations done
    short = tmp_path / "short.fa"
    short.write_text(">s\nTTTTTGGGGG\nACGTCA\n")
    r = run_cli("internal", short, 3, 5, str(tmp_path) + "/s_")
    assert r.returncode == 0 and iteration_lines(r.stderr) == "Iteration 0: masked 3 occurences of GGG\nIteration 1: masked 3 occurences of TTT\n"
    assert (tmp_path / "s_mask2.fa").read_text() == ">s\nNNNNNNNNNNACGTCA\n"


def test_cli_external(tmp_path, tiny):
    fa = str(EX_PREFIX) + ".fa"
    r = run_cli("external", EX_PREFIX, fa, 50, 1, str(tmp_path) + "/ex_")
    assert r.returncode == 0, r.stderr
    assert r.stdout == "Masked 0 basepairs\n" and (tmp_path / "ex_reps_m1.bed").read_text() == ""
    from uncalled_amd import build_index
    _, _, seqs = build_index.read_fasta(fa)
    assert fasta_records(tmp_path / "ex_masked1.fa")[1] == seqs
    # the tiny reference: repeats to mask
    tgt = tmp_path / "tiny.fa"
    tgt.write_text("".join(">%s\n%s\n" % (n, "\n".join(s[i:i + 70] for i in range(0, len(s), 70))) for n, s in zip(tiny["names"], tiny["seqs"])))
    want, _, iv, total = mn.mask_external(tiny["text"], tiny["seqs"], 50, 5, mc.tiny_counts(tiny, 50))
    r = run_cli("external", tiny["prefix"], tgt, 50, 5, str(tmp_path) + "/t_")
    assert r.returncode == 0, r.stderr
    assert r.stdout == "Masked %d basepairs\n" % total and total > 0
    assert (tmp_path / "t_reps_m5.bed").read_text() == "".join("%s\t%d\t%d\n" % (tiny["names"][c], a, b) for c, a, b in iv)
    hdrs, got = fasta_records(tmp_path / "t_masked5.fa")
    assert hdrs == [">c0", ">c1"] and got == want
