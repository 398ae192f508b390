#!/usr/bin/env python3
"""First measurement of unc_align_batch (profiles/align_first_measurement.txt): kernel time of each stage and of the DTW, from HIP
events on the stream (unc_align_last_timing), warm runs, the median of 5, for 2048 queries of about 1000 events by 1000 k-mers and for
one query of the whole example read.  Needs a GPU:  python tools/dev/align_measure.py"""
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
import torch  # noqa: E402,F401  (one HIP runtime per process: uncalled_amd/__init__.py)
from uncalled_amd import capi  # noqa: E402

CALIB = (1467.61, 6.0, 8192.0)


def measure(name, raw, off, calib, queries, kms, reps=5):
    res = capi.align_batch(raw, off, calib, queries, kms)       # warm: code objects, model table, first touch
    rows, wall = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        res = capi.align_batch(raw, off, calib, queries, kms)
        wall.append((time.perf_counter() - t0) * 1e3)
        rows.append(capi.align_last_timing())
    med = [statistics.median(r[i] for r in rows) for i in range(4)]
    cells = int(sum(int(r["n_kept"]) * k.size for r, k in zip(res, kms)))
    print(f"{name}: {len(queries)} queries, events detected {int(res['n_events'].sum())}, kept {int(res['n_kept'].sum())}, "
          f"k-mers {sum(k.size for k in kms)}, cells {cells:.3e}, statuses {sorted(set(map(int, res['status'])))}")
    for label, m, lo, hi in zip(("slices gathered", "event detection (k_events)", "mask + target + normalisation (k_align_prep)", "DTW (k_dtw)"),
                                med, (min(r[i] for r in rows) for i in range(4)), (max(r[i] for r in rows) for i in range(4))):
        print(f"    {label:46s} kernel ms median {m:9.3f} (min {lo:.3f} max {hi:.3f})")
    print(f"    {'the whole call':46s} wall   ms median {statistics.median(wall):9.3f}   rounds {capi.dtw_last_timing()[1]}")


def main():
    assert torch.cuda.is_available(), "needs a GPU"
    rng = np.random.default_rng(94)
    means = capi.dtw_model_tables()[0]
    rg, of, dg = CALIB
    sigs, kms_of = [], []
    for _ in range(128):            # 128 reads of 600 levels (about 1000 events as the detector cuts them), 16 queries on each
        km = rng.integers(0, 1024, 1000).astype(np.uint16)
        lv = means[km[np.sort(rng.integers(0, 1000, 600))]]
        pa = np.concatenate([x + 1.5 * rng.standard_normal(int(rng.integers(6, 14))) for x in lv])
        sigs.append(np.clip(np.rint(pa * dg / rg - of), 0, 32767).astype(np.int16))
        kms_of.append(km)
    raw = np.concatenate(sigs)
    off = np.cumsum([0] + [s.size for s in sigs]).astype(np.uint64)
    calib = capi.make_calib(128, *CALIB)
    queries = [(r, j, 0) for r in range(128) for j in range(16)]
    measure("2048 queries of about 1000 events x 1000 k-mers", raw, off, calib, queries, [kms_of[r] for r, _, _ in queries])
    ex = np.load(ROOT / "tests" / "golden" / "example_read.npz")
    prefix = ROOT / "tests" / "golden" / "example_index" / "example_ref"
    ix = capi.Index(prefix)
    km = capi.ref_kmers(ix, prefix, 0, 6938, 6976, fwd=False)
    sig = ex["signal"]
    measure("the whole example read on the stretch it maps to", sig, np.array([0, sig.size], np.uint64),
            capi.make_calib(1, float(ex["range"]), float(ex["offset"]), float(ex["digitisation"])), [(0, 0, 0)], [km])


if __name__ == "__main__":
    main()
