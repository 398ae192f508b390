#!/usr/bin/env python3
"""First measurement of unc_dtw_band_batch (profiles/dtw_band_first_measurement.txt): one alignment of 20000 k-mers x 30000 events and
the device-filling 2048 x (1000 x 1000) batch, at W = 32, 128, 512 and with the full matrix (unc_dtw_batch, whose kernel this tree
leaves as it was) on the same inputs.  Kernel time from HIP events (unc_dtw_last_timing), one warm call, then the median of 7; the
bytes of back-pointers held; and whether the band held the full matrix's path (equal score bits).
Needs a GPU:  python tools/dev/dtw_band_measure.py"""
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
import torch  # noqa: E402,F401  (one HIP runtime per process: uncalled_amd/__init__.py)
from uncalled_amd import capi  # noqa: E402

from dtw_measure import batch  # noqa: E402


def measure(name, evs, kms, prm, band, reps=7, full=None):
    res, _ = capi.dtw_batch(evs, kms, prm, paths=True, band=band, full=True)          # warm
    ms, wall = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        capi.dtw_batch(evs, kms, prm, paths=True, band=band)
        wall.append((time.perf_counter() - t0) * 1e3)
        k, rounds, held = capi.dtw_last_timing()
        ms.append(k)
    m = statistics.median(ms)
    same = "" if full is None else f"  scores equal to the full matrix's: {int((res['score'].view(np.uint32) == full['score'].view(np.uint32)).sum())} of {len(evs)}"
    against = "" if full is None else f"  full / banded kernel time {full['ms'] / m:7.1f}"
    print(f"{name:34s} {'W = %-4d' % band if band else 'full    '} kernel ms median {m:9.3f} (min {min(ms):.3f} max {max(ms):.3f})  call ms median "
          f"{statistics.median(wall):9.3f}  rounds {rounds}  back-pointer bytes {held:>11d}{against}{same}", flush=True)
    return dict(score=res["score"].copy(), ms=m)


def main():
    assert torch.cuda.is_available(), "needs a GPU"
    rng = np.random.default_rng(94)
    means = capi.dtw_model_tables()[0]
    one = batch([(20000, 30000)], rng, means)
    many = batch([(1000, 1000)] * 2048, rng, means)
    for cost, cname in ((capi.DTW_R94P, "r94p"), (capi.DTW_R94D, "r94d")):
        prm = capi.DTW_EVENT_GLOB.with_cost(cost)
        for name, (evs, kms) in ((f"one 20000 k-mers x 30000 events, {cname}", one), (f"2048 alignments 1000 x 1000, {cname}", many)):
            full = measure(name, evs, kms, prm, 0)
            for band in (32, 128, 512):
                measure(name, evs, kms, prm, band, full=full)


if __name__ == "__main__":
    main()
