"""First measurement of k_dtw_adapt against k_dtw_band (profiles/dtw_adapt_first_measurement.txt): kernel milliseconds by HIP events
(capi.dtw_last_timing), two warm calls, then the median of 7 (of 3 for the batch).  Run from the repository root on one MI355X:
python tools/dev/dtw_adapt_measure.py [OUT.txt]"""
import statistics
import sys
sys.path.insert(0, "."); sys.path.insert(0, "tests")
import numpy as np
from uncalled_amd import capi
import dtw_cases as dc
from dtw_adapt_check import adapt_crumb_bytes

means = capi.dtw_model_tables()[0]
out = open(sys.argv[1] if len(sys.argv) > 1 else "dtw_adapt_measure.txt", "w")
def say(*a):
    line = " ".join(str(x) for x in a)
    print(line, flush=True); out.write(line + "\n"); out.flush()

def timed(fn, reps=7, warm=2):
    for _ in range(warm): fn()
    ms, held = [], 0
    for _ in range(reps):
        fn(); t = capi.dtw_last_timing(); ms.append(t[0]); held = t[2]
    return statistics.median(ms), min(ms), max(ms), held

rows, cols = 20000, 30000
rng = np.random.default_rng(32)
km = rng.integers(0, 1024, rows).astype(np.uint16)
ev = dc.follow(rng, means, km, cols)
prm = capi.DTWParams(0, dc.R94P, 2.0, 1.0, 100.0)
for cost, name in ((dc.R94P, "r94p"), (dc.R94D, "r94d")):
    prm = capi.DTWParams(0, cost, 2.0, 1.0, 100.0)
    W = 64
    m, lo, hi, held = timed(lambda: capi.dtw_batch([ev], [km], prm, paths=False, band=W))
    cells_band = cols * (2 * W + 1)
    say(f"{name} 20000 x 30000 k_dtw_band W=64: median {m:.2f} ms (min {lo:.2f}, max {hi:.2f}), {held} bytes, ~{cells_band} cells, {cells_band / m / 1e3:.1f} Mcells/s")
    band_rate = cells_band / m
    for B in (64, 128, 256):
        m, lo, hi, held = timed(lambda: capi.dtw_batch([ev], [km], prm, paths=False, adaptive=B))
        res, _ = capi.dtw_batch([ev], [km], prm, paths=False, adaptive=B, full=True)
        cells = (rows + cols - 1) * B
        say(f"{name} 20000 x 30000 k_dtw_adapt B={B}: median {m:.2f} ms (min {lo:.2f}, max {hi:.2f}), {held} bytes (formula {adapt_crumb_bytes(rows, cols, B)}), "
            f"{cells} band cells, {cells / m / 1e3:.1f} Mcells/s, ratio to the fixed band {cells / m / band_rate:.2f}, status {int(res['status'][0])} path_len {int(res['path_len'][0])}")

# a batch of 2000 simulated reads of 3000 to 30000 events, the stretch 1.5 times too long
rng = np.random.default_rng(33)
evs, kms = [], []
for a in range(2000):
    c = int(rng.integers(3000, 30001))
    used = max(5, int(c / 1.5))
    k = rng.integers(0, 1024, int(used * 1.5)).astype(np.uint16)
    kms.append(k); evs.append(dc.follow(rng, means, k[:used], c))
prm = capi.DTWParams(0, dc.R94D, 1.0, 1.0, 1.0)
for B in (128,):
    m, lo, hi, held = timed(lambda: capi.dtw_batch(evs, kms, prm, paths=False, adaptive=B), reps=3, warm=1)
    res, _ = capi.dtw_batch(evs, kms, prm, paths=False, adaptive=B, full=True)
    cells = sum((e.size + k.size - 1) * B for e, k in zip(evs, kms))
    st = np.bincount(res["status"].astype(int), minlength=8)
    say(f"r94d batch of 2000 reads (3000..30000 events) k_dtw_adapt B={B}: median {m:.1f} ms (min {lo:.1f}, max {hi:.1f}), {held} bytes held, "
        f"{cells} band cells, {cells / m / 1e6:.2f} Gcells/s, statuses ok {st[0]} ref_end {st[7]} left_band {st[6]}")
