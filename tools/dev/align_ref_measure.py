#!/usr/bin/env python3
"""First measurement of unc_align_ref_batch (profiles/align_ref_first_measurement.txt): the host wall time of the route by k-mer arrays
(a capi.ref_kmers call per query, then capi.align_batch) beside that of capi.align_ref_batch on the same queries, and the kernel time of
k_ref_kmers (unc_align_ref_last_timing) beside the DTW's.  Warm calls, the median of 5 with min and max.  Two batches on a random
reference built in a temporary directory: the 2048 queries of tools/dev/align_measure.py (about 1000 events by 1000 k-mers), and 256
queries the size of whole reads (20 000 k-mers each) with band = 128.  Needs a GPU:  python tools/dev/align_ref_measure.py"""
import statistics
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
import torch  # noqa: E402,F401  (one HIP runtime per process: uncalled_amd/__init__.py)
from uncalled_amd import build_index, capi  # noqa: E402

CALIB = (1467.61, 6.0, 8192.0)


def signal_of(rng, means, km):
    """samples that dwell 6..13 long on the level of every k-mer in turn"""
    rg, of, dg = CALIB
    pa = np.repeat(means[km], rng.integers(6, 14, km.size)).astype(np.float32)
    pa += 1.5 * rng.standard_normal(pa.size).astype(np.float32)
    return np.clip(np.rint(pa * dg / rg - of), 0, 32767).astype(np.int16)


def spans(xs):
    return f"median {statistics.median(xs):10.3f} (min {min(xs):.3f} max {max(xs):.3f})"


def measure(name, ix, rs, prefix, raw, off, calib, queries, stretches, opts, reps=5):
    def old():
        kms = [capi.ref_kmers(ix, prefix, *s) for s in stretches]
        t1 = time.perf_counter()
        return capi.align_batch(raw, off, calib, queries, kms, opts=opts), t1

    def new():
        return capi.align_ref_batch(rs, raw, off, calib, queries, stretches, opts=opts)
    want, _ = old()
    got = new()         # (both warm now)
    assert want.tobytes() == got.tobytes(), "the two routes disagree"
    w_old, w_loop, w_new, k_ms, dtw_ms = [], [], [], [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        _, t1 = old()
        w_old.append((time.perf_counter() - t0) * 1e3)
        w_loop.append((t1 - t0) * 1e3)
        t0 = time.perf_counter()
        new()
        w_new.append((time.perf_counter() - t0) * 1e3)
        k_ms.append(capi.align_ref_last_timing())
        dtw_ms.append(capi.align_last_timing()[3])
    n_km = sum(max(0, en - st - 4) for _, st, en, _ in stretches)
    print(f"{name}: {len(queries)} queries, k-mers {n_km}, columns {int(got['n_kept'].sum())}, statuses {sorted(set(map(int, got['status'])))}")
    print(f"    {'ref_kmers loop + align_batch':40s} wall   ms {spans(w_old)}")
    print(f"    {'    of which the ref_kmers loop':40s} wall   ms {spans(w_loop)}")
    print(f"    {'align_ref_batch':40s} wall   ms {spans(w_new)}")
    print(f"    {'k_ref_kmers':40s} kernel ms {spans(k_ms)}")
    print(f"    {'DTW (k_dtw), same calls':40s} kernel ms {spans(dtw_ms)}")
    print(f"    k_ref_kmers / DTW = {100 * statistics.median(k_ms) / statistics.median(dtw_ms):.3f} %;  the layout predicts "
          f"{n_km / 4 / 1e6:.3f} MB read, {2 * n_km / 1e6:.3f} MB written: {(n_km / 4 + 2 * n_km) / 1e6 / statistics.median(k_ms):.1f} GB/s at the median")


def main():
    assert torch.cuda.is_available(), "needs a GPU"
    rng = np.random.default_rng(95)
    means = capi.dtw_model_tables()[0]
    with tempfile.TemporaryDirectory() as d:
        n_ref = 400000
        codes = rng.integers(0, 4, n_ref)
        seq = "".join(np.array(list("ACGT"))[codes])
        (Path(d) / "r.fa").write_text(">r\n%s\n" % seq)
        prefix = str(Path(d) / "r")
        build_index.build_from_fasta(str(Path(d) / "r.fa"), prefix)
        ix = capi.Index(prefix)
        rs = capi.RefSeq(ix, prefix)
        print(f"reference: {n_ref} bases, packed copy on the device {rs.device_bytes()} bytes")
        for name, n_reads, per_read, n_km, band in (("2048 queries of about 1000 events x 1000 k-mers", 128, 16, 1000, 0),
                                                    ("256 queries of whole reads, band 128", 256, 1, 20000, 128)):
            starts = rng.integers(0, n_ref - n_km - 4, n_reads)
            stretch_of = [(0, int(s), int(s) + n_km + 4, bool(r & 1)) for r, s in enumerate(starts)]
            sigs = [signal_of(rng, means, capi.ref_kmers(ix, prefix, *s)) for s in stretch_of]
            raw = np.concatenate(sigs)
            off = np.cumsum([0] + [s.size for s in sigs]).astype(np.uint64)
            calib = capi.make_calib(n_reads, *CALIB)
            queries = [(r, j, 0) for r in range(n_reads) for j in range(per_read)]
            measure(name, ix, rs, prefix, raw, off, calib, queries, [stretch_of[r] for r, _, _ in queries], capi.align_opts(band=band))
        rs.close()


if __name__ == "__main__":
    main()
