"""tests/fm_naive.py -- the plain FM index the device's FM layer is compared with (tests/parity_cases.py: case_fm_tiny and its
kin) -- pinned on the CPU: on the bundled `bwa index` files it agrees with the oracle (minibwa, itself pinned on the reference) on
the k-mer ranges, random backward steps and every SA row, and its self-alignment hashes to the digest the reference's own
self_align gave (tests/golden/uncl_goldens.json)."""
import json
from pathlib import Path

import numpy as np
import pytest

from tests import fm_naive
from tests.test_index_params import _digest

GOLD = json.loads((Path(__file__).resolve().parent / "golden" / "uncl_goldens.json").read_text())


@pytest.fixture(scope="module")
def example_fm(example):
    pac = np.fromfile(str(example["prefix"]) + ".pac", dtype=np.uint8)
    i = np.arange(10000)
    codes = ((pac[i >> 2] >> ((~i & 3) << 1)) & 3).astype(np.uint8)
    return fm_naive.NaiveFM(codes)


def test_naive_tables_equal_the_bundled_index_files(example, example_fm):
    bwt = np.fromfile(str(example["prefix"]) + ".bwt", dtype=np.uint64, count=5)
    assert int(bwt[0]) == example_fm.primary and [int(x) for x in bwt[1:5]] == example_fm.L2[1:]


def test_naive_equals_oracle_on_the_bundled_index(oracle_lib, example, example_fm):
    fm = example_fm
    oix = oracle_lib.Index(example["prefix"])
    assert int(oix.size) == fm.n
    assert np.array_equal(fm.kmer_ranges(), oix.kmer_ranges())
    rng = np.random.default_rng(4)
    s = rng.integers(1, fm.n + 1, 2000)
    e = np.minimum(fm.n, s + np.where(rng.integers(0, 2, 2000) == 0, rng.integers(0, 40, 2000), rng.integers(0, fm.n, 2000)))
    c = rng.integers(0, 4, 2000)
    s[:8] = [1, 1, fm.primary + 1, fm.primary, fm.primary + 1, fm.n, 2, 129]
    e[:8] = [1, fm.n, fm.primary + 1, fm.primary, fm.n, fm.n, 128, 130]
    ws, we = fm.get_neighbors(s, e, c)
    for i in range(2000):
        want = fm.get_neighbor(int(s[i]), int(e[i]), int(c[i]))
        assert want == (int(ws[i]), int(we[i]))
        assert oix.get_neighbor(int(s[i]), int(e[i]), int(c[i])) == want, (s[i], e[i], c[i])
    rows = fm.sa_rows()
    assert [oix.sa(k) for k in range(fm.n + 1)] == [int(x) for x in rows]
    assert fm.sa(0) == fm_naive.NO_ROW and fm.sa(fm.primary) == 0


def test_naive_self_align_hashes_to_the_reference_digest(example_fm):
    tr = example_fm.self_align()
    assert len(tr) == 10000
    cap = max(len(x) for x in tr)
    lens = np.zeros((len(tr), cap), dtype=np.uint64)
    for i, x in enumerate(tr):
        lens[i, :len(x)] = x
    assert _digest(lens, [len(x) for x in tr]) == GOLD["example"]["self_align_dist1_sha256"]
