"""CPU: repeat masking below the GPU -- the checker (tests/mask_naive.py) against what the reference's own mask_kmers.py printed
(tests/golden/mask_goldens.npz) and against tests/fm_naive.py's interval sizes, then k_mask.hip and unc_mask.cpp under the lanesim
emulator (tests/lanesim/Makefile.mask, a make file of its own) on the cases of tests/mask_cases.py, which tests/test_gpu_mask.py runs
on the GPU; and the host side's argument checks as a stand-alone program under the address and undefined-behaviour sanitizers."""
import subprocess

import numpy as np
import pytest

import mask_cases as mc
import mask_naive as mn
from conftest import EX_PREFIX, GOLD, ROOT, build_lock, locked_make


@pytest.fixture(scope="module")
def sim_mask_lib():
    from uncalled_amd import capi
    locked_make("-C", str(ROOT / "tests" / "lanesim"), "-f", "Makefile.mask")
    return capi.load(ROOT / "tests" / "lanesim" / "_build_mask" / "libuncalled_sim_mask.so")


@pytest.fixture(scope="module")
def tiny(tmp_path_factory):
    """the tiny reference, its index files, its text as the index holds it, and the checker's window counts, made once"""
    return mc.make_tiny(tmp_path_factory.mktemp("mask_tiny"))


tiny_counts = mc.tiny_counts


def test_checker_reproduces_the_reference_script():
    g = np.load(GOLD / "mask_goldens.npz")
    assert g["name"].size >= 5 and int(g["count"].max()) == 38 and int(g["count"].min()) == 0
    for name, fasta, kmer, out, count in zip(g["name"], g["fasta"], g["kmer"], g["stdout"], g["count"]):
        assert mn.mask_fasta_text(str(fasta), str(kmer)) == (str(out), int(count)), name


def test_checker_on_the_cases_that_state_their_report():
    stated = [c for c in mc.internal_cases() if "report" in c]
    assert len(stated) >= 6
    for c in stated:
        assert mn.mask_internal(c["contigs"], c["k"], c["iters"])[1] == c["report"], c["name"]


def test_checker_window_counts_equal_the_plain_fm_index(tiny):
    """substring counts over the text unpacked from .pac = the size of the interval a backward search ends with"""
    from fm_naive import NaiveFM
    from uncalled_amd import build_index as bi
    codes, _, _ = bi.encode_contigs(tiny["seqs"])
    fm = NaiveFM(codes, [len(s) for s in tiny["seqs"]])
    assert "".join(mn.BASES[c] for c in fm.t) == tiny["text"]
    counts = tiny_counts(tiny, 50)
    c0 = tiny["seqs"][0]
    seen = set()
    for p in list(range(0, len(c0) - 50, 37)) + [c0.index(tiny["parts"]["s6"]), c0.index(tiny["parts"]["pal"]), c0.index(tiny["parts"]["s2"]) + 70]:
        w = c0[p:p + 50]
        s, e = fm.L2[mn.BASES.index(w[-1])] + 1, fm.L2[mn.BASES.index(w[-1]) + 1]
        for ch in reversed(w[:-1]):
            s, e = fm.get_neighbor(s, e, mn.BASES.index(ch))
        assert max(0, e - s + 1) == counts[0][p], p
        seen.add(counts[0][p])
    assert {1, 2, 6} <= seen


def test_tiny_reference_holds_what_the_cases_need(tiny):
    counts, seqs, parts = tiny_counts(tiny, 120), tiny["seqs"], tiny["parts"]
    assert counts[0][seqs[0].index(parts["s1"])] == 1 and counts[0][seqs[0].index(parts["s2"])] == 2
    assert counts[0][seqs[0].index(parts["s6"])] == 6 and counts[1][seqs[1].index(mc.revcomp(parts["s6"]))] == 6
    assert tiny_counts(tiny, 50)[0][seqs[0].index(parts["pal"])] == 2           # a palindrome is its own reverse strand
    assert "N" * 31 in seqs[1] and parts["s2"].lower() in seqs[1] and 2000 < sum(map(len, seqs)) < 3500


def test_header_declares_the_masking_entry_points_and_the_build_holds_the_sources():
    import re
    import __graft_entry__ as g
    txt = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "uncalled_hip.h").read_text(), flags=re.S)
    syms = set(re.findall(r"\b(unc_mask_[a-z0-9_]+)\s*\(", txt))
    assert syms == {"unc_mask_create", "unc_mask_free", "unc_mask_kmer_counts", "unc_mask_internal", "unc_mask_external", "unc_mask_codes",
                    "unc_mask_last_timing"}
    assert "k_mask.hip" in g.HIP_SOURCES and "unc_mask.cpp" in g.HIP_SOURCES


def test_cli_parses_both_modes():
    from uncalled_amd.__main__ import get_parser
    a = get_parser().parse_args(["mask", "internal", "ref.fa", "10", "30", "out/"])
    assert (a.subcmd, a.mask_mode, a.reference, a.k, a.iters, a.out_prefix) == ("mask", "internal", "ref.fa", 10, 30, "out/")
    a = get_parser().parse_args(["mask", "external", "full", "tgt.fa", "50", "5", "out/"])
    assert (a.mask_mode, a.index_prefix, a.target, a.min_len, a.min_copy, a.out_prefix) == ("external", "full", "tgt.fa", 50, 5, "out/")


@pytest.mark.lanesim
@pytest.mark.parametrize("case", mc.internal_cases(), ids=lambda c: c["name"])
def test_internal_masking_under_the_emulator(case, sim_mask_lib):
    from uncalled_amd import capi
    mc.check_internal(capi, case, lib=sim_mask_lib)


@pytest.mark.lanesim
def test_arguments_and_lifecycle_under_the_emulator(sim_mask_lib):
    from uncalled_amd import capi
    mc.check_arguments(capi, lib=sim_mask_lib)
    mc.check_lifecycle(capi, lib=sim_mask_lib)


@pytest.mark.lanesim
def test_python_layer_under_the_emulator(sim_mask_lib, tmp_path):
    """uncalled_amd.mask on a FASTA file: headers, case and IUPAC letters kept, the report in k-mer strings"""
    from uncalled_amd import mask
    fa = tmp_path / "in.fa"
    fa.write_text(">one first\nACG\n>six x y\nNNacgNN\nACGnAC\nGRY\n>seven\nacN\n")
    r = mask.mask_internal(str(fa), 3, 4, lib=sim_mask_lib)
    assert r["headers"] == [">one first", ">six x y", ">seven"]
    assert r["seqs"] == ["NNN", "NNNNNNNNNNnNNNRY", "acN"] and r["report"] == [("ACG", 4, 12)]


@pytest.mark.lanesim
@pytest.mark.parametrize("fm32", [True, False], ids=["fm32", "64-bit"])
@pytest.mark.parametrize("min_len", [2, 50, 120])
def test_external_masking_of_the_tiny_reference_under_the_emulator(min_len, fm32, tiny, sim_mask_lib):
    from uncalled_amd import capi
    ix = mc.load_index(capi, tiny["prefix"], sim_mask_lib, fm32=fm32)
    out = mc.check_external(capi, ix, tiny["text"], tiny["seqs"], min_len, (1, 5), lib=sim_mask_lib, naive_counts=tiny_counts(tiny, min_len))
    if min_len == 50:
        m1, m5 = out[1][0], out[5][0]
        s6_at, pal_at, s2_at, s1_at = (tiny["seqs"][0].index(tiny["parts"][k]) for k in ("s6", "pal", "s2", "s1"))
        assert m1[0][s6_at:s6_at + 120] == "N" * 120 and m1[0][pal_at:pal_at + 50] == "N" * 50 and m1[0][s2_at:s2_at + 120] == "N" * 120
        assert "N" not in m1[0][s1_at:s1_at + 120]
        assert m5[0][s6_at:s6_at + 120] == "N" * 120 and "N" not in m5[0][s2_at:s2_at + 120] and "N" not in m5[0][pal_at:pal_at + 50]
    ix.close()


@pytest.mark.lanesim
def test_every_kernel_goes_round_its_grid_stride_loop_under_the_emulator(tiny, sim_mask_lib, monkeypatch):
    from uncalled_amd import capi
    monkeypatch.setenv("UNC_MASK_BLOCKS", "2")
    mc.check_grid_strides(capi, tiny, lib=sim_mask_lib)


@pytest.mark.lanesim
@pytest.mark.parametrize("fm32", [True, False], ids=["fm32", "64-bit"])
def test_external_masking_of_a_subset_and_across_junctions_under_the_emulator(fm32, tiny, sim_mask_lib):
    from uncalled_amd import capi
    ix = mc.load_index(capi, tiny["prefix"], sim_mask_lib, fm32=fm32)
    mc.check_external_arguments(capi, ix, lib=sim_mask_lib)
    subset = [tiny["seqs"][1][60:700]]
    mc.check_external(capi, ix, tiny["text"], subset, 50, (1, 5), lib=sim_mask_lib)
    targets = mc.junction_targets(tiny["text"], tiny["seqs"])
    counts = mn.window_counts(tiny["text"], targets, 50)
    half, strand_w = len(tiny["text"]) // 2, targets[0][4:54]
    assert counts[0][4] == 1 and strand_w not in tiny["text"][:half] and strand_w not in tiny["text"][half:]      # only across the junction
    assert counts[1][0] == 1 and targets[1] not in tiny["seqs"][0] and targets[1] not in tiny["seqs"][1]
    mc.check_external(capi, ix, tiny["text"], targets, 50, (1,), lib=sim_mask_lib, naive_counts=counts)
    ix.close()


@pytest.mark.lanesim
@pytest.mark.parametrize("fm32", [True, False], ids=["fm32", "64-bit"])
def test_external_masking_of_the_example_reference_under_the_emulator(fm32, sim_mask_lib):
    """the bundled 10 kb index against its own FASTA: no window of 50 bases occurs twice, nothing is masked"""
    from uncalled_amd import build_index, capi
    _, _, seqs = build_index.read_fasta(str(EX_PREFIX) + ".fa")
    ix = mc.load_index(capi, EX_PREFIX, sim_mask_lib, fm32=fm32)
    out = mc.check_external(capi, ix, mn.pac_text(EX_PREFIX), seqs, 50, (1,), lib=sim_mask_lib)
    assert out[1][2] == 0 and out[1][0] == seqs
    ix.close()


def test_host_side_under_the_sanitizers(tmp_path):
    """tests/mask_host_check.cpp: unc_mask.cpp and k_mask.hip compiled for the CPU against the emulator's runtime, with
    -fsanitize=address,undefined, as a program of its own: every argument check, an empty masker, a small masking run"""
    exe = tmp_path / "mask_host_check"
    sim, csrc = ROOT / "tests" / "lanesim", ROOT / "uncalled_amd" / "csrc"
    with build_lock():
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                        "-Wno-unknown-pragmas", "-I", str(sim), "-I", str(csrc), "-x", "c++", str(ROOT / "tests" / "mask_host_check.cpp"),
                        str(csrc / "unc_mask.cpp"), str(csrc / "k_mask.hip"), str(sim / "lanesim.cpp"), "-o", str(exe), "-lpthread"], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "mask_host_check OK" in r.stdout, r.stdout + r.stderr
