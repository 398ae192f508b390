"""First measurement of repeat masking on the chr20-sized reference as bench.py builds it (chr20_syn: 64.4 Mb, 30 % N-runs; GPU box):
`mask internal` with k = 10 and 30 iterations, `mask external` against the reference's own index with min_len 50 and min_copy 5,
one k-mer count pass, and the same count pass in plain numpy on the
host, the only yardstick there is (the reference's tool chain -- jellyfish, bowtie, bedtools -- is not installed).

    python tools/dev/time_mask.py [out file = profiles/mask_first_measurement.txt] [total bases = 64444167]
"""
import sys
import time
from pathlib import Path
ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
import numpy as np
import torch  # noqa: F401  -- one HIP runtime per process, before the library loads
from uncalled_amd import build_index as small
from uncalled_amd import capi

out_path = Path(sys.argv[1]) if len(sys.argv) > 1 else ROOT / "profiles" / "mask_first_measurement.txt"
total = int(sys.argv[2]) if len(sys.argv) > 2 else 64444167
K, ITERS, MIN_LEN, MIN_COPY = 10, 30, 50, 5
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


names, lens, codes, holes, n_ambs = small.masked_synthetic_genome(1, total, seed=2, name="chr20_syn")
target = codes.copy()
for st, ln, _ in holes:
    target[st:st + ln] = 4
off = np.cumsum([0] + list(lens)).astype(np.uint64)
say("repeat masking, FIRST measurements (nothing here was measured before; no figure was promised)")
say(f"text: chr20_syn, {target.size} bases, {int((target == 4).sum())} of them N ({len(holes)} runs), {len(lens)} contig(s)")


def numpy_count(t, k):
    """every window of k bases without a code 4, first base most significant -> 4^k counters"""
    n = t.size - k + 1
    code = np.zeros(n, dtype=np.int64)
    bad = np.zeros(n, dtype=bool)
    for j in range(k):
        code = (code << 2) | (t[j:j + n] & 3)
        bad |= t[j:j + n] == 4
    return np.bincount(code[~bad], minlength=4 ** k).astype(np.uint32)


t0 = time.time()
want = numpy_count(target, K)
say(f"host, plain numpy, one count pass (k = {K}): {time.time() - t0:8.3f} s wall")

with capi.Masker(target, off) as m:
    ms = []
    for _ in range(4):
        got = m.kmer_counts(K)
        ms.append(m.last_timing()[0])
    assert np.array_equal(got, want), "device counts differ from numpy's"
    say(f"k_kmer_count, one pass (k = {K}): {min(ms[1:]):8.3f} ms kernel (best of 3 after a warm-up; all: " + ", ".join("%.3f" % x for x in ms) +
        ")   counts equal numpy's")

with capi.Masker(target, off) as m:
    t0 = time.time()
    rep = m.internal(K, ITERS)
    wall = time.time() - t0
    c, v, f = m.last_timing()
    after = m.codes()
say(f"internal, k = {K}, {ITERS} iterations asked, {len(rep)} done: {wall:8.3f} s wall; kernels: count + argmax {c:.3f} ms, flag + cover {v:.3f} ms; "
    f"{int((after == 4).sum() - (target == 4).sum())} bases masked; first k-mers " + ", ".join("%d x%d" % (a, b) for a, b, _ in rep[:3]))

prefix = ROOT / "data" / "mask_timing" / "chr20_syn"
if not Path(str(prefix) + ".sa").exists():
    prefix.parent.mkdir(parents=True, exist_ok=True)
    t0 = time.time()
    small.build_from_codes(str(prefix), names, [""] * len(names), lens, codes, holes, n_ambs, sa_device="cuda:0")
    say(f"(index of the same reference built in {time.time() - t0:.1f} s)")
ix = capi.Index(prefix, dense_sa=False)
for tap in (False, True):
    with capi.Masker(target, off) as m:
        t0 = time.time()
        r = m.external(ix, MIN_LEN, MIN_COPY, counts=tap)
        wall = time.time() - t0
        c, v, f = m.last_timing()
        masked = r[0] if tap else r
    say(f"external, own index ({ix.size} rows), min_len {MIN_LEN}, min_copy {MIN_COPY}, count tap {'on ' if tap else 'off'}: {wall:8.3f} s wall; "
        f"kernels: FM look-ups {f:.3f} ms, cover {v:.3f} ms; {masked} bases masked")
ix.close()
out_path.parent.mkdir(parents=True, exist_ok=True)
out_path.write_text("\n".join(lines) + "\n")
