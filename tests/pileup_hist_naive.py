"""TEST INFRASTRUCTURE: the independent checker of the pile-up's level histograms and of the two-sample Kolmogorov-Smirnov distance.
Pure Python: q, the centres and the width as Python integers (pileup_naive.q_of), the bucket by floor division, the distance as
fractions.Fraction over the cumulative counts, and the two doubles by the written operations of include/uncalled_hip.h (int -> float is
round-to-nearest in CPython, math.sqrt is correctly rounded)."""
import math
from fractions import Fraction

import numpy as np

import pileup_naive as pn

BUCKETS = 64


def centre_of(mean):
    """c = rint(float64(float32 mean) * 2^20)"""
    return pn.q_of(mean)


def width_of(width):
    """w = rint(float64(float32 width) * 2^20)"""
    return pn.q_of(width)


def bucket_of(q, c, w):
    t = q - c + 32 * w
    return 0 if t < 0 else min(t // w, BUCKETS - 1)


def level_with_q(q):
    """a float32 level whose q is exactly `q`, or None: q / 2^20 must be a float32 (24 significant bits) below 2048"""
    lv = np.float32(q / pn.ONE)
    return lv if abs(float(lv)) < pn.LIMIT and pn.q_of(lv) == q else None


class Hist:
    """the histograms beside a pileup_naive.Naive: (rid, pos, strand) -> 64 counts; centre: a function of the key"""

    def __init__(self, regions, centre, w, keep_shared=False):
        self.nv = pn.Naive(regions, keep_shared)
        self.centre, self.w = centre, w
        self.rows = {}

    def add(self, rid, pos, fwd, level, smp_n, shared=None):
        n = len(rid)
        shared = [0] * n if shared is None else shared
        self.nv.add(rid, pos, fwd, level, smp_n, shared)
        for r, p, f, lv, sh in zip(np.asarray(rid).tolist(), np.asarray(pos).tolist(), np.asarray(fwd).tolist(),
                                   np.asarray(level, np.float32).tolist(), np.asarray(shared).tolist()):
            if (sh and not self.nv.keep_shared) or not math.isfinite(lv) or abs(lv) >= pn.LIMIT or not self.nv.inside(r, p):
                continue
            key = (r, p, 0 if f else 1)
            self.rows.setdefault(key, [0] * BUCKETS)[bucket_of(pn.q_of(lv), self.centre(key), self.w)] += 1
        return self

    def row(self, key):
        return self.rows.get(key, [0] * BUCKETS)


def ks(row_a, row_b):
    """-> (n_a, n_b, num, bucket, sign, d, ks) of two rows of 64 Python integers, both with a record"""
    n_a, n_b = sum(row_a), sum(row_b)
    assert n_a > 0 and n_b > 0
    A = B = 0
    best, where, sign = Fraction(0), 0, 0
    for k in range(BUCKETS):
        A += row_a[k]
        B += row_b[k]
        diff = Fraction(A, n_a) - Fraction(B, n_b)
        if abs(diff) > best:       # strictly: the lowest bucket keeps a tie
            best, where, sign = abs(diff), k, 1 if diff > 0 else -1
    num = best * n_a * n_b
    assert num.denominator == 1
    num = int(num)
    prod = float(n_a) * float(n_b)
    d = float(num) / prod
    return n_a, n_b, num, where, sign, d, d * math.sqrt(prod / (float(n_a) + float(n_b)))


def products(row_a, row_b):
    """the largest A(k) * n_b and B(k) * n_a the kernel forms"""
    n_a, n_b = sum(row_a), sum(row_b)
    return n_a * n_b       # = A(63) * n_b = B(63) * n_a
