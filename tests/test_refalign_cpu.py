"""CPU: the packed reference on the device below the GPU -- k_refseq.hip (k_ref_kmers) and unc_refseq.cpp (unc_refseq_*,
unc_align_ref_batch) under the lanesim emulator, against unc_ref_kmers, a restatement from the FASTA string, and unc_align_batch.

The two sources are compiled as part of k_align.hip and unc_align.cpp (which include them), so the emulator library that
tests/lanesim/Makefile.align builds holds them and is the one loaded here.

The long stretch (the whole of a 70 000-base reference, 70 runs of 1024 k-mers) runs here as well: under the emulator the call that
holds it and the 5 000 short stretches takes about a second."""
import ctypes

import numpy as np
import pytest

import align_cases as ac
import refalign_cases as rc
from conftest import EX_PREFIX, GOLD, ROOT, locked_make

SIM = ROOT / "tests" / "lanesim" / "_build_align" / "libuncalled_sim_align.so"


@pytest.fixture(scope="module")
def sim():
    from uncalled_amd import capi
    locked_make("-C", str(ROOT / "tests" / "lanesim"), "-f", "Makefile.align")
    return capi.load(SIM)


@pytest.fixture(scope="module")
def G():
    return ac.Goldens()


@pytest.fixture(scope="module")
def example(sim):
    from uncalled_amd import capi
    ix = capi.Index(EX_PREFIX, lib=sim)
    return ix, capi.RefSeq(ix, EX_PREFIX)


def test_library_exports_the_refseq_entry_points():
    import __graft_entry__ as g
    assert "k_refseq.hip" in g.HIP_INCLUDED and "unc_refseq.cpp" in g.HIP_INCLUDED
    L = ctypes.CDLL(str(g.build_hip()))      # hipcc cross-compiles k_refseq.hip for gfx950 without a GPU
    for s in ("unc_refseq_load", "unc_refseq_free", "unc_refseq_device_bytes", "unc_refseq_kmers_batch", "unc_align_ref_batch",
              "unc_align_ref_last_timing"):
        assert hasattr(L, s), s
    from uncalled_amd import capi
    assert capi.REF_STRETCH.itemsize == 24


def test_the_restatement_knows_its_k_mers():
    assert rc.py_kmers("ACGTACG", 0, 7, True).tolist() == [0b0001101100, 0b0110110001, 0b1011000110]
    assert rc.py_kmers("ACGTACG", 0, 7, False).tolist() == rc.py_kmers("CGTACGT", 0, 7, True).tolist()
    assert rc.py_kmers("ACGTACG", 1, 5, True).size == 0


@pytest.mark.lanesim
@pytest.mark.parametrize("m", [0, 1, 2, 3])
def test_tiny_references(sim, tmp_path, m):
    """l_pac % 4 == m: every start 0..8 x every length x both strands x three sequences that start off the bytes' boundaries, one
    call per reference, the rooms apart by gaps of sentinels; the loader's refusals and the argument errors on the same reference"""
    from uncalled_amd import capi
    prefix, seqs = rc.tiny_reference(tmp_path, m)
    ix = capi.Index(prefix, lib=sim)
    l_pac = ix.size // 2
    assert l_pac % 4 == m and l_pac == sum(map(len, seqs))
    rs = capi.RefSeq(ix, prefix)
    assert rs.device_bytes() >= l_pac // 4
    stretches = rc.tiny_stretches([len(s) for s in seqs])
    assert len(stretches) > 900 and (2, len(seqs[2]) - 133, len(seqs[2]), False) in stretches
    assert rc.check_kmers(rs, ix, prefix, stretches, seqs) > 40000
    rc.check_loader(ix, prefix, tmp_path)
    rc.check_kmer_argument_errors(rs, [len(s) for s in seqs])
    rs.close()
    rs.close()


@pytest.mark.lanesim
def test_example_index_k_mers(example):
    from uncalled_amd import capi
    ix, rs = example
    n = ix.seq_len(0)
    stretches = [(0, 0, n, True), (0, 0, n, False)] + [(0, 1000 + i, 1000 + i + 300 + 7 * i, bool(i & 1)) for i in range(64)]
    rc.check_kmers(rs, ix, EX_PREFIX, stretches)
    got = capi.ref_kmers_batch(rs, stretches[:3])
    assert [g.size for g in got] == [n - 4, n - 4, 296] and np.array_equal(got[1], capi.ref_kmers(ix, EX_PREFIX, 0, 0, n, False))


@pytest.mark.lanesim
def test_more_stretches_than_workgroups_and_a_long_one(sim, tmp_path):
    """5 000 stretches of 5..40 bases and the whole of a 70 000-base reference in one call: the emulator's launch has 16 workgroups
    of four wavefronts, the call 5 070 runs.  (The long stretch runs here too: see the module's docstring.)"""
    from uncalled_amd import capi
    prefix, seqs = rc.random_reference(tmp_path, 70000)
    ix = capi.Index(prefix, lib=sim)
    rs = capi.RefSeq(ix, prefix)
    rng = np.random.default_rng(8)
    st = rng.integers(0, 70000 - 40, 5000)
    ln = 5 + np.arange(5000) % 36
    stretches = [(0, int(a), int(a + b), bool(i % 3)) for i, (a, b) in enumerate(zip(st, ln))]
    stretches.insert(2500, (0, 0, 70000, False))
    stretches.append((0, 0, 70000, True))
    got = capi.ref_kmers_batch(rs, stretches)
    for a in (0, 1, 2499, 2500, 2501, 5000, 5001):
        assert np.array_equal(got[a], rc.py_kmers(seqs[0], *stretches[a][1:])), a
    rc.check_kmers(rs, ix, prefix, stretches[:200] + stretches[2400:2600] + stretches[-200:])


@pytest.mark.lanesim
def test_align_ref_batch_equals_align_batch_fed_ref_kmers(G, example):
    ix, rs = example
    assert rc.check_contract(G, rs, ix, EX_PREFIX, ix.seq_len(0), small=True) > 200


@pytest.fixture(scope="module")
def multi(sim, tmp_path_factory):
    from uncalled_amd import capi
    prefix, seqs = rc.multi_reference(tmp_path_factory.mktemp("multi"))
    ix = capi.Index(prefix, lib=sim)
    return ix, capi.RefSeq(ix, prefix), prefix, [len(s) for s in seqs]


@pytest.mark.lanesim
def test_align_ref_batch_on_later_sequences(G, multi):
    ix, rs, prefix, lens = multi
    assert [ix.seq_len(r) for r in range(5)] == lens
    assert rc.check_multi(G, rs, ix, prefix, lens, small=True) > 100


@pytest.mark.lanesim
def test_align_argument_errors_write_nothing(G, example):
    ix, rs = example
    rc.check_align_argument_errors(G, rs, ix, EX_PREFIX, ix.seq_len(0))


@pytest.mark.lanesim
def test_no_queries_and_the_timing(G, example):
    from uncalled_amd import capi
    ix, rs = example
    res = capi.align_ref_batch(rs, G.raw, G.offsets, G.calib, [(0, 1000, 1400)], [(0, 100, 144, False)])
    assert int(res[0]["status"]) == capi.DTW_OK and capi.align_ref_last_timing(rs.L) > 0
    assert capi.align_ref_batch(rs, G.raw, G.offsets, G.calib, [], []).size == 0 and capi.align_ref_last_timing(rs.L) == 0


def test_paf_queries(tmp_path, capsys):
    """--paf's reader: columns, the sample range from base coordinates, unmapped and too short lines, the later line wins"""
    from uncalled_amd.__main__ import clip_paf_queries, load_paf_queries
    paf = tmp_path / "x.paf"
    paf.write_text("a\t900\t9\t450\t+\tchr\t5000\t100\t700\t60\t601\t255\n"
                   "u\t900\t*\t*\t*\t*\t*\t*\t*\t*\t*\t255\n"
                   "s\t900\t9\t450\t-\tchr\t5000\t100\t104\t4\t5\t255\n"
                   "b\t900\t0\t20\t-\tchr\t5000\t7\t12\t5\t6\t255\tmt:f:1.5\n"
                   "a\t900\t10\t451\t-\tchr2\t5000\t101\t701\t60\t601\t255\n"
                   "a\t900\t*\t*\t*\t*\t*\t*\t*\t*\t*\t255\n")
    q = load_paf_queries(str(paf))
    assert "Skipping s" in capsys.readouterr().err
    assert set(q) == {"a", "b"}
    assert q["a"] == dict(smp_st=88, smp_en=4009, ref="chr2", ref_st=101, ref_en=701, fwd=False)
    assert q["b"] == dict(smp_st=0, smp_en=178, ref="chr", ref_st=7, ref_en=12, fwd=False)
    clip_paf_queries(q, [("a", np.zeros(4000, np.int16), None), ("b", np.zeros(4000, np.int16), None)])
    assert q["a"]["smp_en"] == 4000 and q["b"]["smp_en"] == 178


@pytest.mark.lanesim
def test_the_cli_reads_a_paf_under_the_emulator(sim, tmp_path, capsys, monkeypatch):
    """`dtw --paf` in this process with the emulator build in the library's place: the same line as the equivalent query file gives"""
    from uncalled_amd import capi
    from uncalled_amd.__main__ import main
    monkeypatch.setattr(capi, "DEFAULT_LIB", SIM)
    rid = str(np.load(GOLD / "example_read.npz")["read_id"])
    name = capi.Index(EX_PREFIX, lib=sim).seq_names()[0]
    qf, paf = tmp_path / "q.txt", tmp_path / "q.paf"
    qf.write_text("%s 10000 14000 %s 6700 7000 -\n" % (rid, name))
    paf.write_text("%s\t3562\t1125\t1575\t-\t%s\t10000\t6700\t7000\t30\t301\t255\n"
                   "nobody\t100\t*\t*\t*\t*\t*\t*\t*\t*\t*\t255\n"
                   "short\t100\t0\t50\t+\t%s\t10000\t10\t14\t4\t5\t255\n" % (rid, name, name))
    out = []
    for args in ([str(qf)], [str(paf), "--paf"], [str(paf), "--paf", "--band", "64"]):
        main(["dtw", str(EX_PREFIX), str(GOLD / "example_read.fast5")] + args)
        cap = capsys.readouterr()
        out.append(cap.out.strip().split("\n"))
        assert ("Skipping short" in cap.err) == ("--paf" in args)
    assert len(out[0]) == 1 and len(out[1]) == 1 and out[0][0].split("\t")[:2] == out[1][0].split("\t")[:2] and out[0][0].startswith(rid)
    assert len(out[2]) == 1 and out[2][0].startswith(rid)
