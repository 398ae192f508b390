#!/usr/bin/env python3
"""First measurement of unc_dtw_batch (profiles/dtw_first_measurement.txt): GPU cells/s of the mixed batch of tests/test_gpu_dtw.py
and of one large alignment, kernel time from HIP events (unc_dtw_last_timing), warm runs, the median of 7; and the bytes of
back-pointers per cell.  Needs a GPU:  python tools/dev/dtw_measure.py"""
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
import torch  # noqa: E402,F401  (one HIP runtime per process: uncalled_amd/__init__.py)
from uncalled_amd import capi  # noqa: E402


def batch(shapes, rng, means):
    evs, kms = [], []
    for rows, cols in shapes:
        km = rng.integers(0, 1024, rows).astype(np.uint16)
        evs.append((means[km[np.sort(rng.integers(0, rows, cols))]] + 1.5 * rng.standard_normal(cols)).astype(np.float32))
        kms.append(km)
    return evs, kms


def measure(name, evs, kms, prm, reps=7):
    cells = sum(e.size * k.size for e, k in zip(evs, kms))
    for paths in (True, False):
        capi.dtw_batch(evs, kms, prm, paths=paths)          # warm: code object, model table, first touch
        ms, wall = [], []
        for _ in range(reps):
            t0 = time.perf_counter()
            capi.dtw_batch(evs, kms, prm, paths=paths)
            wall.append((time.perf_counter() - t0) * 1e3)
            k, rounds, held = capi.dtw_last_timing()
            ms.append(k)
        m = statistics.median(ms)
        print(f"{name:34s} paths={int(paths)} cells {cells:.3e}  kernel ms median {m:9.3f} (min {min(ms):.3f} max {max(ms):.3f})  "
              f"{cells / m / 1e6:8.3f} Gcells/s  call ms median {statistics.median(wall):9.3f}  rounds {rounds}  "
              f"back-pointer bytes/cell {held / cells:.4f}")


def main():
    assert torch.cuda.is_available(), "needs a GPU"
    rng = np.random.default_rng(94)
    means = capi.dtw_model_tables()[0]
    shapes = [(6000, 4000), (3000, 4500), (2500, 2000), (1, 1), (1, 300), (300, 1), (64, 64), (65, 1000), (1000, 65), (63, 17)]
    shapes += [(int(r), int(c)) for r, c in zip(rng.integers(2, 1200, 62), rng.integers(2, 1200, 62))]
    mixed = batch(shapes, rng, means)
    for cost, cname in ((capi.DTW_R94P, "r94p"), (capi.DTW_R94D, "r94d")):
        prm = capi.DTW_EVENT_GLOB.with_cost(cost)
        measure(f"mixed batch, 72 alignments, {cname}", *mixed, prm)
        measure(f"one alignment 6000 x 4000, {cname}", *batch([(6000, 4000)], rng, means), prm)
        measure(f"one alignment 30000 x 20000, {cname}", *batch([(30000, 20000)], rng, means), prm, reps=5)
        measure(f"2048 alignments 1000 x 1000, {cname}", *batch([(1000, 1000)] * 2048, rng, means), prm, reps=5)


if __name__ == "__main__":
    main()
