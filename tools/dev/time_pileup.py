"""First measurement of the signal pile-up's kernels: k_pileup_accum over the caller's arrays (unc_pileup_add) and the three launches
of unc_pileup_covered, on two inputs -- records spread evenly over every bin of the reference, and all records in 64 bins (the
hot-spot case: amplicon data).  Kernel milliseconds from HIP events (unc_pileup_last_timing, unc_pileup_covered_last_timing), warm
runs, the median of 10; bytes per second against what a record and a bin move at the least.

    python tools/dev/time_pileup.py [out file = profiles/pileup_first_measurement.txt] [records = 4194304] [index prefix = the example's]
"""
import sys
from pathlib import Path
ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
import numpy as np
import torch  # noqa: F401  -- one HIP runtime per process, before the library loads
from uncalled_amd import capi

out_path = Path(sys.argv[1]) if len(sys.argv) > 1 else ROOT / "profiles" / "pileup_first_measurement.txt"
N = int(sys.argv[2]) if len(sys.argv) > 2 else 1 << 22
PREFIX = Path(sys.argv[3]) if len(sys.argv) > 3 else ROOT / "tests" / "golden" / "example_index" / "example_ref"
WARM, REPS = 3, 10
RECORD_IN = 4 + 8 + 4 + 4 + 4           # rid, pos, fwd, level, smp_n read per record (no shared array)
RECORD_ATOMIC = 4 * 8                   # n, S, SS_lo, D: four 64-bit atomics per record (SS_hi only on a carry)
BIN = 40
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def stats(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2], "median %.3f  min %.3f  max %.3f" % (xs[len(xs) // 2], xs[0], xs[-1])


def main():
    assert torch.cuda.is_available(), "needs a GPU"
    index = capi.Index(PREFIX)
    refseq = capi.RefSeq(index, PREFIX)
    seq_len = int(index.seq_len(0))
    rng = np.random.default_rng(23)
    say("signal pile-up (k_pileup_accum, k_pileup_count / _scan / _write), FIRST measurements (nothing here was measured before; no figure was promised)")
    say("machine: %s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
    say("command: python tools/dev/time_pileup.py   (%d records a call, %d warm-up calls, then %d timed)" % (N, WARM, REPS))
    level = rng.normal(90, 12, N).astype(np.float32)
    dwell = rng.integers(1, 60, N).astype(np.uint32)
    fwd = rng.integers(0, 2, N).astype(np.uint32)
    rid = np.zeros(N, np.int32)
    inputs = (("spread: positions uniform over sequence 0 (%d bases)" % seq_len, rng.integers(0, seq_len - 4, N).astype(np.uint64)),
              ("hot spot: 32 positions x 2 strands = 64 bins", (seq_len // 2 + rng.integers(0, 32, N)).astype(np.uint64)))
    for name, pos in inputs:
        pu = capi.Pileup(refseq)
        ms = []
        for i in range(WARM + REPS):
            pu.add(rid, pos, fwd, level, dwell)
            if i >= WARM:
                ms.append(pu.last_timing())
        assert pu.counters() == (0, 0, N * (WARM + REPS))
        med, txt = stats(ms)
        say("%s; table %d bins = %.2f MB" % (name, pu.n_bins(), pu.n_bins() * BIN / 1e6))
        say("   k_pileup_accum, ms:                   %s" % txt)
        say("   at the median: %.1f M records/s, %.1f GB/s of records read, %.1f GB/s of 64-bit atomics" % (
            N / med / 1e3, N * RECORD_IN / med / 1e6, N * RECORD_ATOMIC / med / 1e6))
        for min_cov in (1, 10 ** 9):
            rows = []
            for i in range(WARM + REPS):
                bins, full = pu.covered(min_cov, cap=pu.n_bins())
                if i >= WARM:
                    rows.append(pu.covered_last_timing())
            parts = [stats([r[j] for r in rows]) for j in range(3)]
            say("   covered(min_cov = %d): %d of %d bins" % (min_cov, full, pu.n_bins()))
            for label, (m, t) in zip(("k_pileup_count", "k_pileup_scan ", "k_pileup_write"), parts):
                say("      %s, ms:                 %s" % (label, t))
            say("      count and write each read the table's %.2f MB: %.1f and %.1f GB/s at the medians" % (
                pu.n_bins() * BIN / 1e6, pu.n_bins() * BIN / parts[0][0] / 1e6, pu.n_bins() * BIN / parts[2][0] / 1e6 if parts[2][0] else 0))
        pu.close()
    say("not measured: tables of hundreds of MB (a bacterial genome), the round mode behind k_align_segments at scale, a struct-of-arrays table, more than one GPU")
    out_path.write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
