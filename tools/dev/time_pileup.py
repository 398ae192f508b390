"""First measurement of the signal pile-up's kernels: k_pileup_accum over the caller's arrays (unc_pileup_add) and the three launches
of unc_pileup_covered, on two inputs -- records spread evenly over every bin of the reference, and all records in 64 bins (the
hot-spot case: amplicon data).  Kernel milliseconds from HIP events (unc_pileup_last_timing, unc_pileup_covered_last_timing), warm
runs, the median of 10; bytes per second against what a record and a bin move at the least.

    python tools/dev/time_pileup.py [out file = profiles/pileup_first_measurement.txt] [records = 4194304] [index prefix = the example's]

With --hist as the first argument: the first measurement of the level histograms (k_pileup_hist.hip) on the same two inputs, in ONE
process -- k_pileup_accum without a histogram in this tree's library and, if --parent-lib names one, in the parent commit's, the two
alternating call by call, then the same with a histogram attached, then k_pileup_ks over all covered bins.

    python tools/dev/time_pileup.py --hist [--parent-lib PATH] [out file = profiles/pileup_hist_first_measurement.txt] [records = 4194304]
"""
import sys
from pathlib import Path
ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
import numpy as np
import torch  # noqa: F401  -- one HIP runtime per process, before the library loads
from uncalled_amd import capi

HIST = len(sys.argv) > 1 and sys.argv[1] == "--hist"
if HIST:
    del sys.argv[1]
PARENT_LIB = None
if len(sys.argv) > 2 and sys.argv[1] == "--parent-lib":
    PARENT_LIB = Path(sys.argv[2])
    del sys.argv[1:3]
out_path = Path(sys.argv[1]) if len(sys.argv) > 1 else ROOT / "profiles" / ("pileup_hist_first_measurement.txt" if HIST else "pileup_first_measurement.txt")
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


HIST_REPS = 15
HIST_WIDTH = 0.25


def hist_main():
    assert torch.cuda.is_available(), "needs a GPU"
    branch = capi.load()
    parent = capi.load(PARENT_LIB) if PARENT_LIB else None
    rng = np.random.default_rng(23)           # the records of the first measurement
    say("level histograms of the pile-up (the add in k_pileup_accum, k_pileup_ks), FIRST measurements (nothing here was measured before; no figure was promised)")
    say("machine: %s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
    say("command: python tools/dev/time_pileup.py --hist%s   (%d records a call; one process; per input %d warm-up rounds, then %d timed; a round is one"
        " call of every variant in turn, the order rotating round by round)" % (" --parent-lib <the parent commit's library>" if parent else "", N, WARM, HIST_REPS))
    level = rng.normal(90, 12, N).astype(np.float32)
    dwell = rng.integers(1, 60, N).astype(np.uint32)
    fwd = rng.integers(0, 2, N).astype(np.uint32)
    rid = np.zeros(N, np.int32)
    held = {}
    for L, tag in ((parent, "parent"), (branch, "branch")):
        if L is not None:
            index = capi.Index(PREFIX, lib=L)
            held[tag] = (index, capi.RefSeq(index, PREFIX))
    seq_len = int(held["branch"][0].seq_len(0))
    inputs = (("spread: positions uniform over sequence 0 (%d bases)" % seq_len, rng.integers(0, seq_len - 4, N).astype(np.uint64)),
              ("hot spot: 32 positions x 2 strands = 64 bins", (seq_len // 2 + rng.integers(0, 32, N)).astype(np.uint64)))
    for name, pos in inputs:
        variants = []
        if parent:
            variants.append(("parent, no histogram ", capi.Pileup(held["parent"][1], lib=parent)))
        variants.append(("branch, no histogram ", capi.Pileup(held["branch"][1], lib=branch)))
        with_hist = capi.Pileup(held["branch"][1], lib=branch)
        with_hist.enable_hist(HIST_WIDTH)
        variants.append(("branch, histogram    ", with_hist))
        ms = {label: [] for label, _ in variants}
        for i in range(WARM + HIST_REPS):
            for label, pu in variants[i % len(variants):] + variants[:i % len(variants)]:       # the order rotates round by round
                pu.add(rid, pos, fwd, level, dwell)
                if i >= WARM:
                    ms[label].append(pu.last_timing())
        say("%s; table %d bins = %.2f MB, histograms %.2f MB" % (name, with_hist.n_bins(), with_hist.n_bins() * BIN / 1e6, with_hist.n_bins() * 256 / 1e6))
        med = {}
        for label, pu in variants:
            assert pu.counters() == (0, 0, N * (WARM + HIST_REPS))
            med[label], txt = stats(ms[label])
            say("   k_pileup_accum, %s ms:   %s   (%.1f M records/s at the median)" % (label, txt, N / med[label] / 1e3))
        if parent:
            lo, hi = min(ms["parent, no histogram "]), max(ms["parent, no histogram "])
            m = med["branch, no histogram "]
            say("   branch without a histogram: median %.3f ms %s the parent's own %.3f .. %.3f ms of this run" % (m, "lies within" if lo <= m <= hi else "lies OUTSIDE", lo, hi))
            a, b = variants[0][1], variants[1][1]
            cov = b.covered(1)
            assert a.gather(cov).tobytes() == b.gather(cov).tobytes(), "the two libraries' tables differ"
        say("   with a histogram: %.2f times the time without one; %.1f GB/s of 32-bit atomics more" % (
            med["branch, histogram    "] / med["branch, no histogram "], N * 4 / med["branch, histogram    "] / 1e6))
        cov = with_hist.covered(1)
        rows = with_hist.hist(cov)
        assert np.array_equal(rows.sum(axis=1, dtype=np.uint64), with_hist.gather(cov)["n"]), "a bin's buckets do not sum to its n"
        # k_pileup_ks: a second sample, half a level higher, over every covered bin
        other = capi.Pileup(held["branch"][1], lib=branch)
        other.enable_hist(HIST_WIDTH)
        other.add(rid, pos, fwd, level + np.float32(0.5), dwell)
        both = with_hist.covered(1, other=other)
        ks_ms = []
        for i in range(WARM + HIST_REPS):
            got = with_hist.ks(other, both)
            if i >= WARM:
                ks_ms.append(with_hist.ks_last_timing())
        m, txt = stats(ks_ms)
        say("   k_pileup_ks over %d covered bins, ms:        %s   (%.1f GB/s of rows read at the median; d from %.4f to %.4f)" % (
            both.size, txt, both.size * 512 / m / 1e6, float(got["d"].min()), float(got["d"].max())))
        for _, pu in variants:
            pu.close()
        other.close()
    say("not measured: histograms of hundreds of MB, the round mode behind k_align_segments at scale, a bucket-major layout, hot bins privatised in LDS, more than one GPU")
    out_path.write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    hist_main() if HIST else main()
