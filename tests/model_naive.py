"""TEST INFRASTRUCTURE: the independent checker of the training accumulator.  Pure Python with arbitrary-precision integers:
q = rint(float64(level) * 2^20) (round to nearest even), the sums as Python ints, finish by the formulas of include/uncalled_hip.h
with math.sqrt(float(V)) (int -> float is round-to-nearest in CPython, math.sqrt is correctly rounded)."""
import math

import numpy as np

NK = 1024
ONE = 2 ** 20
LIMIT = 2048.0


def q_of(level):
    return int(np.rint(np.float64(np.float32(level)) * ONE))


def accumulate(kmers, levels, shared=None, keep_shared=False, into=None):
    """-> dict(n, S, SS: lists of 1024 Python ints, dropped)"""
    acc = into or dict(n=[0] * NK, S=[0] * NK, SS=[0] * NK, dropped=0)
    kmers = np.asarray(kmers).ravel()
    levels = np.asarray(levels, np.float32).ravel()
    shared = np.zeros(kmers.size, np.uint32) if shared is None else np.asarray(shared).ravel()
    for k, lv, sh in zip(kmers.tolist(), levels.tolist(), shared.tolist()):
        if sh and not keep_shared:
            continue
        if not math.isfinite(lv) or abs(lv) >= LIMIT:
            acc["dropped"] += 1
            continue
        q = q_of(lv)
        acc["n"][k] += 1
        acc["S"][k] += q
        acc["SS"][k] += q * q
    return acc


def of_read(read):
    """ModelAcc.read()'s tuple -> the same dict"""
    n, S, lo, hi, dropped = read
    return dict(n=[int(x) for x in n], S=[int(x) for x in S], SS=[(int(h) << 64) | int(l) for l, h in zip(lo, hi)], dropped=int(dropped))


def finish(acc, prior_pairs, min_obs):
    """-> (float32 (1024, 2) pairs, k-mers kept from the prior)"""
    out = np.array(prior_pairs, np.float32).reshape(NK, 2).copy()
    kept = 0
    for k in range(NK):
        n, S, SS = acc["n"][k], acc["S"][k], acc["SS"][k]
        V = n * SS - S * S
        assert V >= 0
        if n < max(min_obs, 2) or V == 0:
            kept += 1
            continue
        out[k, 0] = np.float32(float(S) / float(n) / 1048576.0)
        out[k, 1] = np.float32(math.sqrt(float(V)) / float(n) / 1048576.0)
    return out, kept
