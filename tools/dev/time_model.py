"""First measurement of the training reduction (k_model_accum): one batch of 2 048 queries of the shape `dtw --paf` produces on the
example data (the example read's PAF line, 2 048 copies), two routes to the same per-k-mer sums:
  A  capi.align_ref_batch with an accumulator and no segment outputs: the records never leave the device;
  B  capi.align_ref_batch(segments=True, kmers=True), what the parent of the accumulator offers: every 40-byte record and the
     k-mers copied to the host, then n, S and SS summed there -- tests/model_naive.py's arithmetic in numpy, SS in two 64-bit words.
The sums of both routes are compared before anything is printed.

    python tools/dev/time_model.py [out file = profiles/model_first_measurement.txt] [queries = 2048]
"""
import sys
import tempfile
import time
from pathlib import Path
ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
import numpy as np
import torch  # noqa: F401  -- one HIP runtime per process, before the library loads
from uncalled_amd import __main__ as cli
from uncalled_amd import _uncalled_amd as unc
from uncalled_amd import capi

out_path = Path(sys.argv[1]) if len(sys.argv) > 1 else ROOT / "profiles" / "model_first_measurement.txt"
N = int(sys.argv[2]) if len(sys.argv) > 2 else 2048
WARM, REPS = 3, 10
G = ROOT / "tests" / "golden"
PREFIX = G / "example_index" / "example_ref"
FAST5 = G / "example_read.fast5"
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def stats(xs):
    xs = sorted(xs)
    return "median %.3f  min %.3f  max %.3f" % (xs[len(xs) // 2], xs[0], xs[-1])


def example_paf_line():
    conf = unc.Conf()
    conf.bwa_prefix = str(PREFIX)
    pool = unc.MapPool(conf)
    pool.add_fast5(str(FAST5))
    out = []
    while pool.running():
        out += pool.update()
    pool.stop()
    return str(out[0])


def host_sums(kms, segs, info):
    """n, S, SS (low and high word) per k-mer of the records of a batch, as the accumulator counts them without KEEP_SHARED"""
    km = np.concatenate([k[int(i["row_first"]):int(i["row_first"]) + s.size] for k, s, i in zip(kms, segs, info)])
    sg = np.concatenate(segs)
    keep = (sg["shared"] == 0) & np.isfinite(sg["level"]) & (np.abs(sg["level"]) < 2048)
    km = km[keep]
    q = np.rint(sg["level"][keep].astype(np.float64) * 2.0 ** 20).astype(np.int64)
    n = np.bincount(km, minlength=1024).astype(np.uint64)
    S = np.zeros(1024, np.int64)
    np.add.at(S, km, q)
    # q * q < 2^62 as 2^32 * hi32 + lo32 parts: the parts' sums stay below 2^64 for fewer than 2^32 records
    qq = (q * q).astype(np.uint64)
    lo32, hi32 = np.zeros(1024, np.uint64), np.zeros(1024, np.uint64)
    np.add.at(lo32, km, qq & np.uint64(0xFFFFFFFF))
    np.add.at(hi32, km, qq >> np.uint64(32))
    SS = [int(h) * 2 ** 32 + int(l) for l, h in zip(lo32, hi32)]
    return n, S, SS


paf = Path(tempfile.mkdtemp(prefix="time_model_")) / "example.paf"
paf.write_text(example_paf_line() + "\n")
queries = cli.load_paf_queries(str(paf))
reads = cli.load_query_reads(unc, str(FAST5), queries)
cli.clip_paf_queries(queries, reads)
rid, raw, cal = reads[0]
q = queries[rid]
index = capi.Index(PREFIX)
refseq = capi.RefSeq(index, PREFIX)
calib = capi.make_calib(1, 0, 0, 1)
calib[0] = cal
raw = np.asarray(raw, np.int16)
offsets = np.array([0, raw.size], np.uint64)
qs = [(0, q["smp_st"], q["smp_en"])] * N
stretches = [(index.seq_names().index(q["ref"]), q["ref_st"], q["ref_en"], q["fwd"])] * N
opts = capi.align_opts(max_events=50000)

say("training reduction (k_model_accum), FIRST measurements (nothing here was measured before; no figure was promised)")
prop = torch.cuda.get_device_properties(0)
say("machine: one %s (%s, %d CUs), HIP runtime %s, torch %s" % (prop.name, prop.gcnArchName, prop.multi_processor_count, torch.version.hip,
                                                               torch.__version__))
say("command: python tools/dev/time_model.py")
say("batch: %d queries in one call, each samples [%d, %d) of the example read against %d reference bases (%d k-mers), DTWr94d, "
    "full matrix; %d warm-up calls, then %d timed, per route" % (N, q["smp_st"], q["smp_en"], q["ref_en"] - q["ref_st"],
                                                                 q["ref_en"] - q["ref_st"] - 4, WARM, REPS))

acc = capi.ModelAcc()
a_acc, a_seg, a_wall = [], [], []
for rep in range(WARM + REPS):
    acc.reset()
    t0 = time.perf_counter()
    capi.align_ref_batch(refseq, raw, offsets, calib, qs, stretches, opts=opts, accumulate=acc)
    wall = (time.perf_counter() - t0) * 1e3
    if rep >= WARM:
        a_acc.append(acc.last_timing())
        a_seg.append(capi.align_segments_last_timing())
        a_wall.append(wall)
dev_n, dev_S, dev_lo, dev_hi, dropped = acc.read()

b_seg, b_wall, b_host = [], [], []
for rep in range(WARM + REPS):
    t0 = time.perf_counter()
    res, kms, segs, info = capi.align_ref_batch(refseq, raw, offsets, calib, qs, stretches, opts=opts, kmers=True, segments=True)
    wall = (time.perf_counter() - t0) * 1e3
    t1 = time.perf_counter()
    n, S, SS = host_sums(kms, segs, info)
    host = (time.perf_counter() - t1) * 1e3
    if rep >= WARM:
        b_seg.append(capi.align_segments_last_timing())
        b_wall.append(wall)
        b_host.append(host)

assert np.array_equal(n, dev_n) and np.array_equal(S, dev_S) and dropped == 0
assert SS == [(int(h) << 64) | int(l) for l, h in zip(dev_lo, dev_hi)]
say("records of the batch: %d counted, %d dropped; the sums of both routes are equal (n, S and the 128-bit SS of all 1024 k-mers)"
    % (int(dev_n.sum()), dropped))
say("A  accumulator on the device, no segment outputs")
say("   unc_model_acc_last_timing, ms:        " + stats(a_acc))
say("   unc_align_segments_last_timing, ms:   " + stats(a_seg))
say("   wall of the call, ms:                 " + stats(a_wall))
say("B  records and k-mers copied out (the route without the accumulator), summed with numpy on the host")
say("   unc_align_segments_last_timing, ms:   " + stats(b_seg))
say("   wall of the call, ms:                 " + stats(b_wall))
say("   host sums (n, S, SS), ms:             " + stats(b_host))
say("not measured: long reads (thousands of rows a query), batches of several rounds, more than one GPU")
out_path.write_text("\n".join(lines) + "\n")
