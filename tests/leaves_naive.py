"""TEST INFRASTRUCTURE: plain references for the leaf bench (tests/leaves_cases.py).  Integers only: every comparison against
them is exact equality.  Nothing here looks at the kernels' sources; each function states the operation in a few lines of numpy or
a Python loop."""
import functools

import numpy as np

U64 = np.uint64
M64 = (1 << 64) - 1
M32 = (1 << 32) - 1


# ---- sorts and merges ----
def sort64(keys):
    return np.sort(np.asarray(keys, dtype=U64))


def merge64(a, b):
    return np.sort(np.concatenate([np.asarray(a, dtype=U64), np.asarray(b, dtype=U64)]))


def wk_lt(x, y):
    """map_sort_wide.h, wk_lt: (a, b) in this order"""
    return x[0] < y[0] or (x[0] == y[0] and x[1] < y[1])


def key_gt(x, y):
    """map_sort.h, key_gt, of the legacy network: a first, b where a ties"""
    return x[0] > y[0] or (x[0] == y[0] and x[1] > y[1])


def sort128(keys, legacy=False):
    """keys: uint64 [n, 2] = (a, b).  Sorted by a plain comparison sort under the leaf's own order, restated above."""
    keys = np.asarray(keys, dtype=U64).reshape(-1, 2)
    rows = [(int(a), int(b)) for a, b in keys]
    if legacy:
        cmp = lambda x, y: 1 if key_gt(x, y) else (-1 if key_gt(y, x) else 0)
    else:
        cmp = lambda x, y: -1 if wk_lt(x, y) else (1 if wk_lt(y, x) else 0)
    rows.sort(key=functools.cmp_to_key(cmp))
    return np.array(rows, dtype=U64).reshape(-1, 2)


def merge128(a, b):
    return sort128(np.concatenate([np.asarray(a, dtype=U64).reshape(-1, 2), np.asarray(b, dtype=U64).reshape(-1, 2)]))


def ranks128(*arrays):
    """distinct 128-bit keys -> their ranks (1-based) in the (a, b) order, one array per input: the wide cases' reference then
    works on plain integers"""
    allk = np.concatenate([np.asarray(x, dtype=U64).reshape(-1, 2) for x in arrays])
    order = np.lexsort((allk[:, 1], allk[:, 0]))
    rank = np.empty(len(allk), dtype=np.int64)
    rank[order] = np.arange(1, len(allk) + 1)
    out, at = [], 0
    for x in arrays:
        n = len(np.asarray(x).reshape(-1, 2))
        out.append(rank[at:at + n])
        at += n
    return out


def split(a, b, d):
    """how many of the first d keys of merge(a, b) come from a (a, b ascending, all keys distinct)"""
    if d == 0:
        return 0
    merged = np.sort(np.concatenate([a, b]))
    return int(np.searchsorted(a, merged[d - 1], side="right"))


# ---- repair ----
def repair(run, lt=None):
    """A key strictly smaller than the largest key before it in its run is a misfit.  -> (indices kept, indices of the misfits),
    both in the run's order.  lt: the order (default: integers)"""
    lt = lt or (lambda x, y: x < y)
    kept, misfits, top = [], [], None
    for i, k in enumerate(run):
        if top is not None and lt(k, top):
            misfits.append(i)
        else:
            kept.append(i)
            if top is None or lt(top, k):
                top = k
    return kept, misfits


# ---- wave primitives: v, head of 64 lanes ----
def seg_incl_max(v, head):
    out, run = [], 0
    for i in range(64):
        run = int(v[i]) if (i == 0 or head[i]) else max(run, int(v[i]))
        out.append(run)
    return np.array(out, dtype=U64)


def excl_sum(v, mask=M32):
    """-> (exclusive prefix sums, total), wrapping like the unsigned type"""
    out, s = [], 0
    for i in range(64):
        out.append(s)
        s = (s + int(v[i])) & mask
    return np.array(out, dtype=U64), s


def excl_max(v):
    out, m = [], 0
    for i in range(64):
        out.append(m)
        m = max(m, int(v[i]))
    return np.array(out, dtype=U64), m


def prefix_popc(mask):
    return np.array([bin(int(mask) & ((1 << l) - 1)).count("1") for l in range(64)], dtype=U64)


def wave_sum64(v):
    return sum(int(x) for x in v) & M64
