"""TEST INFRASTRUCTURE: the independent checker of the signal pile-up.  Pure Python with arbitrary-precision integers and dictionaries
keyed (rid, pos, strand) (strand 0 = plus, 1 = minus): q = rint(float64(level) * 2^20) (round to nearest even), the sums as Python
ints, the statistics by the formulas of include/uncalled_hip.h with math.sqrt(float(V)) (int -> float is round-to-nearest in CPython,
math.sqrt is correctly rounded).  Regions are (rid, st, en) triples; the bins are numbered by a plain walk over the sorted regions."""
import math

import numpy as np

ONE = 2 ** 20
LIMIT = 2048.0
K = 5


def q_of(level):
    return int(np.rint(np.float64(np.float32(level)) * ONE))


class Naive:
    def __init__(self, regions, keep_shared=False):
        self.regions = sorted((int(r), int(s), int(e)) for r, s, e in regions)
        self.keep_shared = keep_shared
        self.bins = {}          # (rid, pos, strand) -> [n, S, SS, D]
        self.dropped = self.outside = self.added = 0

    def inside(self, rid, pos):
        return any(r == rid and st <= pos < en - (K - 1) for r, st, en in self.regions)

    def add(self, rid, pos, fwd, level, smp_n, shared=None):
        n = len(rid)
        shared = [0] * n if shared is None else shared
        for r, p, f, lv, d, sh in zip(np.asarray(rid).tolist(), np.asarray(pos).tolist(), np.asarray(fwd).tolist(),
                                      np.asarray(level, np.float32).tolist(), np.asarray(smp_n).tolist(), np.asarray(shared).tolist()):
            if sh and not self.keep_shared:
                continue
            if not math.isfinite(lv) or abs(lv) >= LIMIT:
                self.dropped += 1
                continue
            if not self.inside(r, p):
                self.outside += 1
                continue
            q = q_of(lv)
            b = self.bins.setdefault((r, p, 0 if f else 1), [0, 0, 0, 0])
            b[0] += 1
            b[1] += q
            b[2] += q * q
            b[3] += int(d)
            self.added += 1
        return self

    def counters(self):
        return self.dropped, self.outside, self.added

    def keys_in_order(self):
        """every bin's key, in bin order: regions sorted, then position, then strand"""
        return [(r, p, s) for r, st, en in self.regions for p in range(st, max(st, en - (K - 1))) for s in (0, 1)]

    def covered(self, min_cov, other=None):
        return [i for i, k in enumerate(self.keys_in_order())
                if self.bins.get(k, [0])[0] >= min_cov and (other is None or other.bins.get(k, [0])[0] >= min_cov)]

    def bin_of(self, key):
        """the index keys_in_order() has for a key, by the same walk without the list (for tables of 10^5 bins and more)"""
        rid, pos, strand = key
        at = 0
        for r, st, en in self.regions:
            n = max(0, en - st - (K - 1))
            if r == rid and st <= pos < st + n:
                return 2 * (at + pos - st) + strand
            at += n
        raise KeyError(key)

    def key_of(self, bin_):
        at = 0
        for r, st, en in self.regions:
            n = max(0, en - st - (K - 1))
            if bin_ // 2 < at + n:
                return r, st + bin_ // 2 - at, bin_ % 2
            at += n
        raise IndexError(bin_)

    def covered_of_bins(self, min_cov, other=None):
        """covered() from the bins that hold something: the same list, in time that goes by their number"""
        return sorted(self.bin_of(k) for k, b in self.bins.items() if b[0] >= min_cov and (other is None or other.bins.get(k, [0])[0] >= min_cov))


def words_of(rec):
    """a PILEUP_WORDS record -> [n, S, SS, D]"""
    return [int(rec["n"]), int(rec["S"]), (int(rec["SS_hi"]) << 64) | int(rec["SS_lo"]), int(rec["D"])]


def moments(b):
    """[n, S, SS, D] -> (mean, sd) in double, one rounding per operation"""
    n, S, SS, _ = b
    V = n * SS - S * S
    assert V >= 0
    return float(S) / float(n) / 1048576.0, math.sqrt(float(V)) / float(n) / 1048576.0


def stats(b, mu, sigma):
    """-> (n, mean, sd, dwell, z); mu, sigma: the model's float32 pair of the bin's k-mer"""
    if b is None or b[0] == 0:
        return 0, 0.0, 0.0, 0.0, 0.0
    mean, sd = moments(b)
    dwell = float(b[3]) / float(b[0])
    z = ((mean - float(np.float32(mu))) / float(np.float32(sigma))) * math.sqrt(float(b[0]))
    return b[0], mean, sd, dwell, z


def compare(a, b):
    """-> (mean_a, mean_b, se2, t)"""
    ma, sa = moments(a)
    mb, sb = moments(b)
    se2 = sa * sa / float(a[0] - 1) + sb * sb / float(b[0] - 1)
    t = (ma - mb) / math.sqrt(se2) if se2 > 0 else 0.0
    return ma, mb, se2, t


def py_kmer(seq, pos, fwd):
    """the bin's 5-mer from the FASTA string, reverse-complemented for the minus strand, first base most significant"""
    s = seq[pos:pos + K]
    if not fwd:
        s = s[::-1].translate(str.maketrans("ACGT", "TGCA"))
    return sum("ACGT".index(c) << (2 * (K - 1 - i)) for i, c in enumerate(s))


def bits(x):
    return np.asarray(x, np.float64).view(np.uint64)
