"""GPU: the packed reference in HBM -- k_ref_kmers and unc_align_ref_batch of the gfx950 library on the cases of
tests/refalign_cases.py (those of tests/test_refalign_cpu.py, with the example read's queries), plus what needs the device: two
threads on streams of their own over one unc_refseq_t, and `dtw --paf` in a child process."""
import subprocess
import sys
import threading

import numpy as np
import pytest

import align_cases as ac
import refalign_cases as rc
from conftest import EX_PREFIX, GOLD, ROOT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def G():
    return ac.Goldens()


@pytest.fixture(scope="module")
def example(hip_lib):
    from uncalled_amd import capi
    ix = capi.Index(EX_PREFIX, lib=hip_lib)
    return ix, capi.RefSeq(ix, EX_PREFIX)


@pytest.mark.parametrize("m", [0, 1, 2, 3])
def test_tiny_references(hip_lib, tmp_path, m):
    from uncalled_amd import capi
    prefix, seqs = rc.tiny_reference(tmp_path, m)
    ix = capi.Index(prefix, lib=hip_lib)
    l_pac = ix.size // 2
    assert l_pac % 4 == m
    rs = capi.RefSeq(ix, prefix)
    assert rs.device_bytes() >= l_pac // 4
    assert rc.check_kmers(rs, ix, prefix, rc.tiny_stretches([len(s) for s in seqs]), seqs) > 40000
    rc.check_loader(ix, prefix, tmp_path)
    rc.check_kmer_argument_errors(rs, [len(s) for s in seqs])
    rs.close()


def test_example_index_k_mers(example):
    ix, rs = example
    n = ix.seq_len(0)
    rc.check_kmers(rs, ix, EX_PREFIX, [(0, 0, n, True), (0, 0, n, False)] + [(0, 1000 + i, 1000 + i + 300 + 7 * i, bool(i & 1)) for i in range(64)])


def test_more_stretches_than_workgroups_and_a_long_one(hip_lib, tmp_path):
    """5 000 stretches of 5..40 bases and the whole of a 70 000-base reference, both strands, in one call: 5 140 runs on a launch
    of at most 1 024 workgroups of four wavefronts"""
    from uncalled_amd import capi
    prefix, seqs = rc.random_reference(tmp_path, 70000)
    ix = capi.Index(prefix, lib=hip_lib)
    rs = capi.RefSeq(ix, prefix)
    rng = np.random.default_rng(8)
    st = rng.integers(0, 70000 - 40, 5000)
    stretches = [(0, int(a), int(a) + 5 + i % 36, bool(i % 3)) for i, a in enumerate(st)]
    stretches.insert(2500, (0, 0, 70000, False))
    stretches.append((0, 0, 70000, True))
    got = capi.ref_kmers_batch(rs, stretches)
    for a in (0, 1, 2499, 2500, 2501, 5000, 5001):
        assert np.array_equal(got[a], rc.py_kmers(seqs[0], *stretches[a][1:])), a
    rc.check_kmers(rs, ix, prefix, stretches[:200] + stretches[2400:2600] + stretches[-200:])


def test_align_ref_batch_equals_align_batch_fed_ref_kmers(G, example):
    ix, rs = example
    assert rc.check_contract(G, rs, ix, EX_PREFIX, ix.seq_len(0), small=False) > 250


@pytest.fixture(scope="module")
def multi(hip_lib, tmp_path_factory):
    from uncalled_amd import capi
    prefix, seqs = rc.multi_reference(tmp_path_factory.mktemp("multi"))
    ix = capi.Index(prefix, lib=hip_lib)
    return ix, capi.RefSeq(ix, prefix), prefix, [len(s) for s in seqs]


def test_align_ref_batch_on_later_sequences(G, multi):
    ix, rs, prefix, lens = multi
    assert [ix.seq_len(r) for r in range(5)] == lens
    assert rc.check_multi(G, rs, ix, prefix, lens, small=False) > 100


def test_align_argument_errors_write_nothing(G, example):
    ix, rs = example
    rc.check_align_argument_errors(G, rs, ix, EX_PREFIX, ix.seq_len(0))


def test_two_threads_share_one_refseq(G, example):
    """each thread on a stream of its own: both get what the calling thread gets alone"""
    import torch
    from uncalled_amd import capi
    ix, rs = example
    members = list(range(G.n))
    queries = [G.query(c) for c in members]
    halves = [rc.golden_stretches(G, members, ix.seq_len(0), fwd) for fwd in (True, False)]
    want = [capi.align_ref_batch(rs, G.raw, G.offsets, G.calib, queries, s, paths=True, kmers=True) for s in halves]
    got, errs = [None, None], []

    def work(t):
        try:
            stream = torch.cuda.Stream()
            for _ in range(3):
                got[t] = capi.align_ref_batch(rs, G.raw, G.offsets, G.calib, queries, halves[t], paths=True, kmers=True, stream=stream.cuda_stream)
        except Exception as e:      # noqa: BLE001
            errs.append(e)
    threads = [threading.Thread(target=work, args=(t,)) for t in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errs, errs
    for t in range(2):
        assert got[t][0].tobytes() == want[t][0].tobytes()
        for a, b in zip(got[t][1] + got[t][2], want[t][1] + want[t][2]):
            assert (a is None and b is None) or np.array_equal(a, b)


def test_the_cli_reads_a_paf(example, tmp_path):
    """`python -m uncalled_amd dtw ... --paf` in a child process, on a PAF written from the example read's mapping ('-' strand,
    bases 6938..6976 of the example reference, tests/golden/ref_goldens.npz): the line that the equivalent query line gives; an
    unmapped line and a line too short in the same file"""
    ix, _ = example
    gold = np.load(GOLD / "ref_goldens.npz")
    gh = dict(zip([str(x) for x in gold["hit_fields"]], gold["ex_hit"]))
    rid = str(np.load(GOLD / "example_read.npz")["read_id"])
    name = ix.seq_names()[0]
    rd_st, rd_en, rf_st, rf_en = (int(gh[k]) for k in ("rd_st", "rd_en", "rf_st", "rf_en"))
    n_smp = int(np.load(GOLD / "example_read.npz")["signal"].size)
    qf, paf = tmp_path / "q.txt", tmp_path / "q.paf"
    qf.write_text("%s %d %d %s %d %d -\n" % (rid, rd_st * 80 // 9, min(n_smp, -(-rd_en * 80 // 9)), name, rf_st, rf_en))
    paf.write_text("nobody\t100\t*\t*\t*\t*\t*\t*\t*\t*\t*\t255\n"
                   "%s\t%d\t%d\t%d\t-\t%s\t%d\t%d\t%d\t%d\t%d\t255\n"
                   "short\t100\t0\t50\t+\t%s\t10000\t10\t14\t4\t5\t255\n"
                   % (rid, int(gh["rd_len"]), rd_st, rd_en, name, int(gh["rf_len"]), rf_st, rf_en, int(gh["matches"]), rf_en - rf_st + 1, name))
    out = []
    for args in ([str(qf)], [str(paf), "--paf"]):
        p = subprocess.run([sys.executable, "-m", "uncalled_amd", "dtw", str(EX_PREFIX), str(GOLD / "example_read.fast5")] + args,
                           cwd=str(ROOT), capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, p.stderr
        assert ("Skipping short" in p.stderr) == ("--paf" in args)
        out.append(p.stdout.strip().split("\n"))
    assert len(out[0]) == 1 and len(out[1]) == 1 and out[0][0].startswith(rid + "\t")
    assert out[0][0].split("\t")[:2] == out[1][0].split("\t")[:2]
