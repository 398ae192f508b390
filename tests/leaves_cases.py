"""TEST INFRASTRUCTURE: the cases of the leaf bench, shared by tests/test_leaves_cpu.py (emulator) and tests/test_gpu_leaves.py
(MI355X).  Each family below builds slots and descriptors for tests/leaves/k_leaves.hip, runs them in ONE launch (a workgroup per
case) and compares what comes back with tests/leaves_naive.py, exactly.

A slot starts as a background of 0xA5 bytes with the inputs written into it, areas GAP bytes apart.  The expected slot is that
slot with the expected output written in, and the WHOLE slot is compared: every byte the leaf had no business writing -- the
background in front of and behind every input and output area, the inputs themselves -- is a canary.  Only the ranges a case
names as `free` (contents the leaf leaves unspecified: the tail of a repaired run, the padding of the legacy network) are left out.

Inputs follow what the leaves assume and k_map guarantees (keys distinct and > 0; check_keys asserts it), except where a case says
that ties are legal for its leaf.

leaf                         kernel (k_leaves.hip)      cases
---------------------------  -------------------------  ------------------------------------------------------------------
seg_incl_max64 / 32          leaf_wave_prims            check_seg_scans
excl_sum_bits<2|3|7>         leaf_wave_prims            check_wave_sums
excl_sum32, excl_max32       leaf_wave_prims            check_wave_sums
prefix_popc, wave_sum64      leaf_wave_prims            check_wave_sums
bcast64/32/f, uniform64      leaf_wave_prims            check_wave_bcasts
sort_any64                   leaf_sort64 (p0 = 0)       check_sort64(pattern), check_sort64_in_place
sort_regs64<1|2|4|8>         leaf_sort64 (p0 = E)       check_sort64_classes (and through sort_any64)
sort_hybrid64                leaf_sort64 (p0 = 9)       check_sort64_classes, check_sort64_in_place
sort_regs<E>, sort_hybrid    leaf_sort128               check_sort128(pattern), check_sort128_classes
merge_runs<4,1>, <1,4>       leaf_merge41 / leaf_merge14  check_merge(kind), check_merge_verify
mergew_runs<4,1>             leaf_mergew41              check_merge("w41")
merge_split<4,1>, <1,4>      leaf_split                 check_splits
mergew_split<4,1>            leaf_split                 check_splits
stage_tile<4,1>, <1,4>       leaf_tile                  check_tiles
stagew_tile, mergew_tile     leaf_tile (p0 = 2)         check_tiles
repair_run, repairw_run      leaf_repair_run            check_repair_run(wide)
repair_runs4                 leaf_repair_runs4          check_repair_runs4
the chain of phase S         leaf_chain                 check_chain(wide)
"""
import numpy as np

import leaves_naive as ln

U64, U32, U8 = np.uint64, np.uint32, np.uint8
BG = 0xA5
GAP = 32
# descriptor words and kernel numbers of k_leaves.hip
D_AADJ, D_ACUM, D_AN, D_BADJ, D_BCUM, D_BN, D_OUT, D_P, D_RET = 0, 6, 12, 13, 17, 21, 22, 23, 30
LK_WAVE, LK_SORT64, LK_SORT128, LK_MERGE41, LK_MERGE14, LK_MERGEW41, LK_SPLIT, LK_TILE, LK_REPAIR_RUN, LK_REPAIR_RUNS4, LK_CHAIN = range(11)
(WP_SEG64, WP_SEG32, WP_SUMB2, WP_SUMB3, WP_SUMB7, WP_SUM32, WP_MAX32, WP_POPC, WP_WSUM64, WP_BCAST64, WP_BCAST32, WP_UNIFORM64,
 WP_BCASTF) = range(13)
MERGE_TILE, MERGEW_TILE, MERGE_MIN = 576, 320, 256
PATTERNS = ("random", "ascending", "descending", "all-equal", "top-bit")
PATTERNS128 = PATTERNS + ("equal-a", "equal-b", "few-a")
SIZES = (1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 1536, 2047, 2048, 2049)


def check_keys(keys):
    """what the leaves assume of their input: keys > 0 and distinct"""
    k = np.asarray(keys, dtype=U64).reshape(-1)
    assert (k > 0).all() and len(np.unique(k)) == len(k)


def check_keys128(keys):
    k = np.asarray(keys, dtype=U64).reshape(-1, 2)
    assert ((k[:, 0] > 0) | (k[:, 1] > 0)).all() and len(np.unique(k, axis=0)) == len(k)


def distinct_keys(rng, n, hi=1 << 62):
    """n distinct even keys in [2, hi), unsorted (odd values stay free for keys a case inserts by hand)"""
    while True:
        k = np.unique(rng.integers(1, hi // 2, size=n + 8, dtype=np.uint64) * U64(2))
        if len(k) >= n:
            return rng.permutation(k)[:n].astype(U64)


class Case:
    """one workgroup's slot, descriptor and expectation"""

    def __init__(self, name):
        self.name = name
        self.desc = np.zeros(32, dtype=U32)
        self.buf = bytearray()
        self.want_writes = []       # (offset, bytes)
        self.free = []              # (offset, length) not compared
        self.post = None            # post(desc, slot): further checks (multisets, returned counts)
        self.want_ret = None

    def put(self, arr, gap=True, align=16):
        """an input area: its byte offset (aligned, GAP bytes of background in front unless gap is False)"""
        if gap:
            self.buf += bytes([BG]) * GAP
        self.buf += bytes([BG]) * (-len(self.buf) % align)
        off = len(self.buf)
        self.buf += np.ascontiguousarray(arr).tobytes()
        return off

    def room(self, nbytes, gap=True, align=16):
        """an area of background for the leaf to write to"""
        return self.put(np.full(nbytes, BG, dtype=U8), gap, align)

    def want(self, off, arr):
        self.want_writes.append((off, np.ascontiguousarray(arr).tobytes()))

    def slot(self):
        b = bytes(self.buf) + bytes([BG]) * GAP
        return np.frombuffer(b + bytes([BG]) * (-len(b) % 16), dtype=U8)

    def set_A(self, adj, cum, n):
        for r, (a, c) in enumerate(zip(adj, cum)):
            self.desc[D_AADJ + r] = a & ln.M32
            self.desc[D_ACUM + r] = c
        self.desc[D_AN] = n

    def set_B(self, adj, cum, n):
        for r, (a, c) in enumerate(zip(adj, cum)):
            self.desc[D_BADJ + r] = a & ln.M32
            self.desc[D_BCUM + r] = c
        self.desc[D_BN] = n

    def p(self, *vals):
        for i, v in enumerate(vals):
            self.desc[D_P + i] = v


def ret64(desc):
    return int(desc[D_RET]) | (int(desc[D_RET + 1]) << 32)


def run_cases(L, kernel, cases):
    """all cases in one launch; the whole slot of each against its expectation"""
    assert cases
    slots_in = [c.slot() for c in cases]
    sb = max(len(s) for s in slots_in)
    slots = np.full((len(cases), sb), BG, dtype=U8)
    for i, s in enumerate(slots_in):
        slots[i, :len(s)] = s
    desc = np.stack([c.desc for c in cases])
    d, got = L.run(kernel, desc, slots)
    for i, c in enumerate(cases):
        want = slots[i].copy()
        for off, b in c.want_writes:
            assert off + len(b) <= len(slots_in[i]), c.name
            want[off:off + len(b)] = np.frombuffer(b, dtype=U8)
        keep = np.ones(sb, dtype=bool)
        for off, n in c.free:
            keep[off:off + n] = False
        bad = np.nonzero((got[i] != want) & keep)[0]
        assert bad.size == 0, "%s: slot differs at bytes %s (first: got word %s, want %s)" % (
            c.name, bad[:8].tolist(), got[i][bad[0] // 8 * 8:bad[0] // 8 * 8 + 8].view(U64), want[bad[0] // 8 * 8:bad[0] // 8 * 8 + 8].view(U64))
        if c.want_ret is not None:
            assert ret64(d[i]) == c.want_ret, "%s: returned %#x, want %#x" % (c.name, ret64(d[i]), c.want_ret)
        keep_desc = np.ones(32, dtype=bool)
        keep_desc[D_RET:] = False
        if kernel == LK_CHAIN:
            keep_desc[[D_P + 4, D_P + 5, D_P + 6, D_AN]] = False
        assert (d[i][keep_desc] == c.desc[keep_desc]).all(), c.name + ": descriptor changed"
        if c.post:
            c.post(d[i], got[i])
    return d, got


# ================================================== wave primitives ==================================================
def wave_case(name, prim, par, v, h, out0, out1=None):
    c = Case(name)
    v = np.asarray(v, dtype=U64)
    h = np.asarray(h, dtype=U32)
    assert v.shape == (64,) and h.shape == (64,)
    c.buf += v.tobytes() + h.tobytes() + bytes([BG]) * 1024
    c.p(prim, par)
    c.want(768, np.asarray(out0, dtype=U64))
    c.want(1280, np.zeros(64, dtype=U64) if out1 is None else np.full(64, out1, dtype=U64))
    return c


def _heads(*lanes):
    h = np.zeros(64, dtype=U32)
    h[list(lanes)] = 1
    return h


def seg_cases(bits):
    rng = np.random.default_rng(6400 + bits)
    prim = WP_SEG64 if bits == 64 else WP_SEG32
    mask = ln.M64 if bits == 64 else ln.M32

    def rnd():
        return rng.integers(0, mask, size=64, dtype=np.uint64, endpoint=True)

    def hi_only():      # only high-word bits (of the 64-bit value; the top half of the 32-bit one)
        return (rng.integers(1, 1 << (bits // 2), size=64, dtype=np.uint64) << U64(bits // 2)) & U64(mask)

    def lo_only():
        return rng.integers(1, 1 << (bits // 2), size=64, dtype=np.uint64)

    head_sets = [("head@%d" % l, _heads(l)) for l in (0, 1, 15, 16, 17, 31, 32, 33, 47, 48, 62, 63)]
    head_sets += [("no-head", _heads()), ("all-heads", np.ones(64, dtype=U32)), ("row-starts", _heads(0, 16, 32, 48)),
                  ("row-ends", _heads(15, 31, 47, 63))]
    cases = []
    for hn, h in head_sets:
        for vn, gen in (("random", rnd), ("hi-only", hi_only), ("lo-only", lo_only)):
            v = gen()
            cases.append(wave_case("seg%d %s %s" % (bits, hn, vn), prim, 0, v, h, ln.seg_incl_max(v, h)))
    # the maximum in the lane just in front of a head (must not cross it), and in lanes 15 / 31 / 47 with readers in the next row
    for p in (0, 14, 15, 16, 30, 31, 32, 46, 47, 48, 61, 62):
        v = rng.integers(1, 1000, size=64, dtype=np.uint64)
        v[p] = mask - 5
        for hn, h in (("head-behind", _heads(p + 1)), ("no-head", _heads()), ("head-at", _heads(p))):
            cases.append(wave_case("seg%d max@%d %s" % (bits, p, hn), prim, 0, v, h, ln.seg_incl_max(v, h)))
    for i in range(200):
        v = rnd() if i % 4 else rng.integers(0, 8, size=64, dtype=np.uint64)         # (every fourth: many ties)
        h = (rng.random(64) < (0.02, 0.1, 0.3, 0.6)[i % 4]).astype(U32)
        cases.append(wave_case("seg%d random %d" % (bits, i), prim, 0, v, h, ln.seg_incl_max(v, h)))
    # the repair's way of calling it: head = (lane == 0), whatever the slot's head words say
    for vn, gen in (("random", rnd), ("hi-only", hi_only), ("lo-only", lo_only), ("random2", rnd)):
        v = gen()
        cases.append(wave_case("seg%d lane0-head %s" % (bits, vn), prim, 1, v, np.ones(64, dtype=U32), ln.seg_incl_max(v, _heads(0))))
    for p in (15, 31, 47, 63, 0):
        v = rng.integers(1, 1000, size=64, dtype=np.uint64)
        v[p] = mask
        cases.append(wave_case("seg%d lane0-head max@%d" % (bits, p), prim, 1, v, _heads(), ln.seg_incl_max(v, _heads(0))))
    return cases


def check_seg_scans(L, bits):
    run_cases(L, LK_WAVE, seg_cases(bits))


def check_wave_sums(L):
    rng = np.random.default_rng(77)
    z = np.zeros(64, dtype=U32)
    cases = []
    for prim, bits in ((WP_SUMB2, 2), (WP_SUMB3, 3), (WP_SUMB7, 7)):
        top = (1 << bits) - 1
        pats = [("all-max", np.full(64, top, dtype=U64)), ("all-zero", np.zeros(64, dtype=U64))]
        for l in (0, 31, 32, 63):
            v = np.zeros(64, dtype=U64)
            v[l] = top
            pats.append(("only-lane-%d" % l, v))
        pats += [("random %d" % i, rng.integers(0, top, size=64, dtype=np.uint64, endpoint=True)) for i in range(100)]
        for name, v in pats:
            pre, tot = ln.excl_sum(v)
            cases.append(wave_case("excl_sum_bits<%d> %s" % (bits, name), prim, 0, v, z, pre, tot))
    pats = [("small %d" % i, rng.integers(0, 9, size=64, dtype=np.uint64)) for i in range(10)]
    pats += [("wraps %d" % i, rng.integers(1 << 30, 1 << 32, size=64, dtype=np.uint64)) for i in range(20)]
    pats += [("all-max", np.full(64, ln.M32, dtype=U64)), ("all-zero", np.zeros(64, dtype=U64))]
    for name, v in pats:
        pre, tot = ln.excl_sum(v)
        assert not name.startswith("wraps") or sum(int(x) for x in v) > ln.M32
        cases.append(wave_case("excl_sum32 " + name, WP_SUM32, 0, v, z, pre, tot))
    pats = [("random %d" % i, rng.integers(0, 1 << 32, size=64, dtype=np.uint64)) for i in range(20)]
    for l in (0, 63, 31, 32):
        v = rng.integers(0, 1000, size=64, dtype=np.uint64)
        v[l] = ln.M32
        pats.append(("max@%d" % l, v))
    pats += [("all-equal", np.full(64, 0x80000001, dtype=U64)), ("all-zero", np.zeros(64, dtype=U64))]
    for name, v in pats:
        pre, tot = ln.excl_max(v)
        cases.append(wave_case("excl_max32 " + name, WP_MAX32, 0, v, z, pre, tot))
    masks = [0, ln.M64, 1 << 31, 1 << 32, 1 << 63, 1, 0xFFFFFFFF, 0xFFFFFFFF00000000] + [int(x) for x in rng.integers(0, ln.M64, size=40, dtype=np.uint64)]
    for m in masks:
        v = rng.integers(0, ln.M64, size=64, dtype=np.uint64)       # (only v[0] is the mask)
        v[0] = m
        cases.append(wave_case("prefix_popc %#x" % m, WP_POPC, 0, v, z, ln.prefix_popc(m)))
    pats = [("random %d" % i, rng.integers(0, ln.M64, size=64, dtype=np.uint64, endpoint=True)) for i in range(20)]
    pats += [("small", rng.integers(0, 100, size=64, dtype=np.uint64)), ("all-max", np.full(64, ln.M64, dtype=U64))]
    for name, v in pats:
        assert name == "small" or sum(int(x) for x in v) > ln.M64        # (wraps)
        cases.append(wave_case("wave_sum64 " + name, WP_WSUM64, 0, v, z, np.full(64, ln.wave_sum64(v), dtype=U64)))
    run_cases(L, LK_WAVE, cases)


def check_wave_bcasts(L):
    rng = np.random.default_rng(78)
    z = np.zeros(64, dtype=U32)
    cases = []
    for rep in range(3):
        hi, lo = rng.integers(1, 1 << 32, size=64, dtype=np.uint64), rng.integers(1, 1 << 32, size=64, dtype=np.uint64)
        v = (hi << U64(32)) | lo
        assert (hi != lo).all()
        for src in (0, 31, 32, 63, 1, 47):
            cases.append(wave_case("bcast64 src %d" % src, WP_BCAST64, src, v, z, np.full(64, v[src], dtype=U64)))
            cases.append(wave_case("bcast32 src %d" % src, WP_BCAST32, src, v, z, np.full(64, v[src] & U64(ln.M32), dtype=U64)))
            f = rng.standard_normal(64).astype(np.float32).view(U32).astype(U64)
            cases.append(wave_case("bcastf src %d" % src, WP_BCASTF, src, f, z, np.full(64, f[src], dtype=U64)))
        cases.append(wave_case("uniform64", WP_UNIFORM64, 0, v, z, np.full(64, v[0], dtype=U64)))
    run_cases(L, LK_WAVE, cases)


# ================================================== narrow sorts ==================================================
def pattern_keys(rng, n, pattern):
    """-> (keys, ties_legal)"""
    if pattern == "random":
        return distinct_keys(rng, n), False
    if pattern == "ascending":
        return np.sort(distinct_keys(rng, n)), False
    if pattern == "descending":
        return np.sort(distinct_keys(rng, n))[::-1].copy(), False
    if pattern == "all-equal":      # ties are legal for the sort
        return np.full(n, 0x0123456789ABCDEF, dtype=U64), True
    if pattern == "top-bit":        # pairs of keys that differ only in bit 63
        half = distinct_keys(rng, (n + 1) // 2)
        k = np.concatenate([half, half | U64(1 << 63)])[:n]
        return rng.permutation(k), False
    raise ValueError(pattern)


def split_counts(rng, n, variant):
    """n keys over six runs, some of them empty (equal `cum` values; a leading and a trailing empty run)"""
    if variant == 0:
        live = [1, 3, 4]            # runs 0, 2 and 5 empty
    elif variant == 1:
        live = [0, 1, 2, 3, 4, 5]
    else:
        live = [2]                  # one run in the middle
    c = [0] * 6
    cuts = np.sort(rng.integers(0, n + 1, size=len(live) - 1)) if len(live) > 1 else np.array([], dtype=np.int64)
    edges = [0] + [int(x) for x in cuts] + [n]
    for j, r in enumerate(live):
        c[r] = edges[j + 1] - edges[j]
    assert sum(c) == n
    return c


def sort64_case(name, keys, mode, ties=False, counts=None, in_place=False):
    """mode: what leaf_sort64 calls (0 = sort_any64).  counts: the six runs apart in the slot; None: the degenerate KeyArr of the
    unsorted run (six equal adj, six cum of 0)"""
    keys = np.asarray(keys, dtype=U64)
    n = len(keys)
    if not ties:
        check_keys(keys)
    c = Case(name)
    if counts is None:
        off = c.put(keys)
        c.set_A([off] * 6, [0] * 6, n)
    else:
        adj, cum, at = [], [], 0
        for r in range(6):
            off = c.put(keys[at:at + counts[r]])
            adj.append(off - 8 * at)
            cum.append(at)
            at += counts[r]
        c.set_A(adj, cum, n)
        assert not in_place
    out = off if in_place else c.room(8 * n)
    c.desc[D_OUT] = out
    c.p(mode)
    c.want(out, ln.sort64(keys))
    return c


def check_sort64(L, pattern):
    rng = np.random.default_rng(sum(map(ord, pattern)))
    cases = []
    for i, n in enumerate(SIZES):
        keys, ties = pattern_keys(rng, n, pattern)
        cases.append(sort64_case("sort_any64 %s n=%d six runs v%d" % (pattern, n, i % 3), keys, 0, ties, counts=split_counts(rng, n, i % 3)))
        if pattern == "random":
            cases.append(sort64_case("sort_any64 random n=%d six runs v%d" % (n, (i + 1) % 3), keys, 0, ties, counts=split_counts(rng, n, (i + 1) % 3)))
            cases.append(sort64_case("sort_any64 random n=%d degenerate KeyArr" % n, keys, 0, ties))
    run_cases(L, LK_SORT64, cases)


def check_sort64_in_place(L):
    """out_off = the run's own offset, exactly n keys of room: the background behind the n keys is the canary that pins the padding
    stored past n (docs/history.md)"""
    rng = np.random.default_rng(31)
    cases = []
    for n in SIZES:
        for pattern in ("random", "descending"):
            keys, _ = pattern_keys(rng, n, pattern)
            cases.append(sort64_case("sort_any64 in place %s n=%d" % (pattern, n), keys, 0, in_place=True))
    for n in (513, 700, 1025, 2049):
        cases.append(sort64_case("sort_hybrid64 in place n=%d" % n, distinct_keys(rng, n), 9, in_place=True))
    run_cases(L, LK_SORT64, cases)


def check_sort64_classes(L):
    """every size class called by name, below, at and (for the hybrid) around its own sizes"""
    rng = np.random.default_rng(32)
    cases = []
    for e in (1, 2, 4, 8):
        for n in sorted({1, 2, 3, 64 * e - 1, 64 * e, 32 * e + 1, 37}):
            if n <= 64 * e:
                cases.append(sort64_case("sort_regs64<%d> n=%d" % (e, n), distinct_keys(rng, n), e, counts=split_counts(rng, n, n % 3)))
    for n in (1, 2, 100, 511, 512, 513, 1024, 1025, 1500):
        cases.append(sort64_case("sort_hybrid64 n=%d" % n, distinct_keys(rng, n), 9, counts=split_counts(rng, n, n % 3)))
    run_cases(L, LK_SORT64, cases)


# ================================================== legacy 128-bit sorts ==================================================
def pattern_keys128(rng, n, pattern):
    if pattern in ("random", "ascending", "descending", "top-bit"):
        a, _ = pattern_keys(rng, n, pattern)
        b = distinct_keys(rng, n, hi=1 << 64)
        return np.stack([a, b], axis=1), False
    if pattern == "all-equal":
        return np.tile(np.array([[0x0123456789ABCDEF, 0xFEDCBA9876543210]], dtype=U64), (n, 1)), True
    if pattern == "equal-a":        # b alone decides
        return np.stack([np.full(n, 1 << 40, dtype=U64), distinct_keys(rng, n, hi=1 << 64)], axis=1), False
    if pattern == "equal-b":
        return np.stack([distinct_keys(rng, n, hi=1 << 64), np.full(n, (1 << 63) + 5, dtype=U64)], axis=1), False
    if pattern == "few-a":          # many ties on a, decided by b
        return np.stack([rng.integers(1, 6, size=n, dtype=np.uint64) << U64(30), distinct_keys(rng, n, hi=1 << 64)], axis=1), False
    raise ValueError(pattern)


def sort_class(n):
    return 1 if n <= 64 else 2 if n <= 128 else 4 if n <= 256 else 8 if n <= 512 else 9


def sort128_case(name, keys, mode, ties=False):
    keys = np.asarray(keys, dtype=U64).reshape(-1, 2)
    n = len(keys)
    if not ties:
        check_keys128(keys)
    c = Case(name)
    off = c.put(keys)
    c.set_A([off], [0], n)
    room = n
    if mode == 9:                   # the legacy hybrid pads its output to a power of two of at least 1024 keys: (+inf, +inf) behind the n keys
        room = 1024
        while room < n:
            room *= 2
    out = c.room(16 * room)
    c.desc[D_OUT] = out
    c.p(mode)
    c.want(out, ln.sort128(keys, legacy=True))
    if room > n:
        c.want(out + 16 * n, np.full(2 * (room - n), ln.M64, dtype=U64))
    return c


def check_sort128(L, pattern):
    rng = np.random.default_rng(sum(map(ord, pattern)) + 128)
    cases = []
    for n in SIZES:
        keys, ties = pattern_keys128(rng, n, pattern)
        cases.append(sort128_case("sort128 %s n=%d" % (pattern, n), keys, sort_class(n), ties))
    run_cases(L, LK_SORT128, cases)


def check_sort128_classes(L):
    rng = np.random.default_rng(33)
    cases = []
    for e in (1, 2, 4, 8):
        for n in sorted({1, 2, 64 * e - 1, 64 * e, 32 * e + 1}):
            if n <= 64 * e:
                cases.append(sort128_case("sort_regs<%d> n=%d" % (e, n), pattern_keys128(rng, n, "few-a")[0], e))
    for n in (2, 512, 513, 1100):
        cases.append(sort128_case("sort_hybrid n=%d" % n, pattern_keys128(rng, n, "few-a")[0], 9))
    run_cases(L, LK_SORT128, cases)


# ================================================== merges ==================================================
def runs4(n, shape):
    """n keys of a sequence over four runs"""
    if shape == "n000":
        return [n, 0, 0, 0]
    if shape == "000n":
        return [0, 0, 0, n]
    if shape == "0-5-0-rest" and n >= 5:
        return [0, 5, 0, n - 5]
    q = n // 4
    return [q, q, q, n - 3 * q]


def merge_inputs(rng, total, split, wide):
    """-> (A, B): ascending, all keys distinct; uint64 [n] or, wide, [n, 2]"""
    if wide:
        a = (rng.integers(1, 40, size=total, dtype=np.uint64) << U64(31))       # many keys tie on a: b decides, across A and B too
        allk = ln.sort128(np.stack([a, distinct_keys(rng, total, hi=1 << 64)], axis=1))
    else:
        allk = np.sort(distinct_keys(rng, total))
    idx = np.arange(total)
    na = max(1, total // 2)
    if split == "A-below-B":
        ia = idx[:na]
    elif split == "B-below-A":
        ia = idx[total - na:]
    elif split == "interleaved":
        ia = idx[0::2]
    elif split == "A-one-key":
        ia = idx[[int(rng.integers(0, total))]]
    elif split == "B-one-key":
        ia = np.delete(idx, int(rng.integers(0, total)))
    elif split == "half":
        ia = idx[rng.random(total) < 0.5]
    elif split == "A-first-tile":   # A is exactly the first tile: a tile boundary on the boundary between the sequences
        ia = idx[:min(total - 1, MERGEW_TILE if wide else MERGE_TILE)]
    else:
        m = rng.random(total) < rng.uniform(0.2, 0.8)
        m[int(rng.integers(0, total))] = True
        ia = idx[m]
        if len(ia) == total:
            ia = ia[:-1]
    ib = np.setdiff1d(idx, ia)
    assert len(ia) >= 1 and len(ib) >= 1
    return allk[ia], allk[ib]


def merge_case(name, kind, four, one, counts, verify=0, ordered=True):
    """kind "41": merge_runs<4,1>(four runs, one run); "14": merge_runs<1,4>(one, four); "w41": mergew_runs<4,1>.  The four-run
    sequence lies run by run, apart; the single run next, and the output area directly behind it (as off_tmp lies behind the streams)"""
    wide = kind == "w41"
    kb = 16 if wide else 8
    c = Case(name)
    if ordered:
        (check_keys128 if wide else check_keys)(np.concatenate([four, one]))
    adj, cum, at = [], [], 0
    for r in range(4):
        off = c.put(four[at:at + counts[r]])
        adj.append(off - kb * at)
        cum.append(at)
        at += counts[r]
    assert at == len(four)
    off1 = c.put(one)
    n = len(four) + len(one)
    out = c.room(kb * n, gap=False, align=kb)
    assert out == off1 + kb * len(one)
    if kind == "14":
        c.set_A([off1], [0], len(one))
        c.set_B(adj, cum, len(four))
    else:
        c.set_A(adj, cum, len(four))
        c.set_B([off1], [0], len(one))
    c.desc[D_OUT] = out
    c.p(verify)
    if ordered:
        c.want(out, ln.merge128(four, one) if wide else ln.merge64(four, one))
        c.want_ret = None if wide else 1
    else:
        c.free.append((out, kb * n))
        c.want_ret = 0
    return c


def merge_cases(kind, verify=0):
    wide = kind == "w41"
    T = MERGEW_TILE if wide else MERGE_TILE
    rng = np.random.default_rng({"41": 41, "14": 14, "w41": 4116}[kind] + verify)
    cases = []
    for total in (T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1, 3 * T + 7):
        for split, shape in (("A-below-B", "even"), ("B-below-A", "even"), ("interleaved", "even"), ("A-one-key", "even"), ("B-one-key", "even"),
                             ("random", "n000"), ("random", "000n"), ("random", "0-5-0-rest"), ("random", "even"), ("A-first-tile", "n000")):
            A, B = merge_inputs(rng, total, split, wide)
            four, one = (B, A) if kind == "14" else (A, B)
            cases.append(merge_case("merge %s total=%d %s runs %s" % (kind, total, split, shape), kind, four, one, runs4(len(four), shape), verify))
        # a tile boundary exactly on the boundary between two runs of the four-run sequence
        A, B = merge_inputs(rng, total, "interleaved", wide)
        four, one = (B, A) if kind == "14" else (A, B)
        first = T // 2 if len(four) > T // 2 else len(four)
        rest = len(four) - first
        cases.append(merge_case("merge %s total=%d run boundary on the tile boundary (interleaved)" % (kind, total), kind, four, one,
                                [first, rest // 2, 0, rest - rest // 2], verify))
        if total > T + 1:
            A, B = merge_inputs(rng, total, "A-below-B", wide)
            four, one = (B, A) if kind == "14" else (A, B)
            if len(four) > T:
                cases.append(merge_case("merge %s total=%d run boundary on the tile boundary (one side)" % (kind, total), kind, four, one,
                                        [T, 0, len(four) - T, 0], verify))
    A, B = merge_inputs(rng, 2, "A-one-key", wide)
    four, one = (B, A) if kind == "14" else (A, B)
    for cnt in ([1, 0, 0, 0], [0, 0, 0, 1], [0, 1, 0, 0]):
        cases.append(merge_case("merge %s 1 + 1 keys runs %s" % (kind, cnt), kind, four, one, cnt, verify))
        cases.append(merge_case("merge %s 1 + 1 keys swapped runs %s" % (kind, cnt), kind, one, four, cnt, verify))
    return cases


def check_merge(L, kind):
    run_cases(L, {"41": LK_MERGE41, "14": LK_MERGE14, "w41": LK_MERGEW41}[kind], merge_cases(kind))


def check_merge_verify(L):
    """merge_runs' own check: 1 on ascending inputs; 0 when one key of A is out of order -- at the start of a tile, in the last lane's
    share of a tile, and straddling two tiles (the previous tile's last key is carried over)"""
    T = MERGE_TILE
    for kind, kern in (("41", LK_MERGE41), ("14", LK_MERGE14)):
        cases = merge_cases(kind, verify=1)
        rng = np.random.default_rng(99)
        for total in (2 * T + 1, 3 * T + 7):
            for at, where in ((T, "start of tile 1"), (T - 2, "last lane of tile 0"), (T - 1, "straddling tiles 0 and 1"), (0, "start of tile 0"),
                              (2 * T - 1, "straddling tiles 1 and 2"), (300, "inside tile 0")):
                allk = np.sort(distinct_keys(rng, total))
                if at + 1 >= total - 1:
                    continue
                four, one = allk[:-1].copy(), allk[-1:]          # the single run: the largest key of all, so that outputs 0 .. total - 2 are `four` as it lies
                four[[at, at + 1]] = four[[at + 1, at]]
                for shape in ("even", "n000"):
                    cases.append(merge_case("merge %s verify: inversion at output %d (%s), total=%d runs %s" % (kind, at, where, total, shape), kind,
                                            four, one, runs4(len(four), shape), verify=1, ordered=False))
        run_cases(L, kern, cases)


def check_splits(L):
    rng = np.random.default_rng(55)
    cases = []
    for which, kind in ((0, "41"), (1, "14"), (2, "w41")):
        wide = kind == "w41"
        T = MERGEW_TILE if wide else MERGE_TILE
        kb = 16 if wide else 8
        for total in (2, 17, T, 2 * T + 1, 3 * T + 7):
            for split, shape in (("A-below-B", "even"), ("B-below-A", "0-5-0-rest"), ("interleaved", "even"), ("A-one-key", "000n"), ("B-one-key", "n000"),
                                 ("random", "even"), ("random", "0-5-0-rest")):
                A, B = merge_inputs(rng, total, split, wide)
                four, one = (B, A) if kind == "14" else (A, B)
                counts = runs4(len(four), shape)
                c = Case("split %s total=%d %s runs %s" % (kind, total, split, shape))
                adj, cum, at = [], [], 0
                for r in range(4):
                    off = c.put(four[at:at + counts[r]])
                    adj.append(off - kb * at)
                    cum.append(at)
                    at += counts[r]
                off1 = c.put(one)
                if kind == "14":
                    c.set_A([off1], [0], len(one)); c.set_B(adj, cum, len(four))
                else:
                    c.set_A(adj, cum, len(four)); c.set_B([off1], [0], len(one))
                first, second = (one, four) if kind == "14" else (four, one)            # (A, B) as the leaf sees them
                ds = sorted({0, 1, len(first), len(second), total, total - 1} | set(range(T, total + 1, T)) | {int(x) for x in rng.integers(0, total + 1, size=6)})
                d_off = c.put(np.array(ds, dtype=U32))
                out = c.room(4 * len(ds))
                c.desc[D_OUT] = out
                c.p(which, d_off, len(ds))
                ra, rb = ln.ranks128(first, second) if wide else (first, second)
                c.want(out, np.array([ln.split(ra, rb, d) for d in ds], dtype=U32))
                cases.append(c)
    run_cases(L, LK_SPLIT, cases)


def check_tiles(L):
    """stage_tile<4,1> and <1,4>: a tile's share of A and B as staged; stagew_tile + mergew_tile: one wide tile staged and merged"""
    rng = np.random.default_rng(56)
    cases = []
    for which, kind in ((0, "41"), (1, "14"), (2, "w41")):
        wide = kind == "w41"
        T = MERGEW_TILE if wide else MERGE_TILE
        kb = 16 if wide else 8
        A, B = merge_inputs(rng, 2 * T + 40, "half", wide)
        four, one = (B, A) if kind == "14" else (A, B)
        first, second = (one, four) if kind == "14" else (four, one)
        la, lb = len(first), len(second)
        shares = [(0, 0, min(la, T // 2), T - min(la, T // 2)), (0, 0, 1, 0), (0, 0, 0, 1), (3, 0, min(T, la - 3), 0), (0, 5, 0, min(T, lb - 5)),
                  (la - 1, lb - 64, 1, 64), (la - 20, lb - 45, 20, 45), (7, 9, 100, T - 101), (la - 1, lb - 1, 1, 1), (10, 10, 63, 1), (10, 10, 1, 64)]
        for shape in ("even", "0-5-0-rest"):
            counts = runs4(len(four), shape)
            for a0, b0, na, nb in shares:
                assert a0 + na <= la and b0 + nb <= lb and 0 < na + nb <= T
                c = Case("tile %s a0=%d b0=%d na=%d nb=%d runs %s" % (kind, a0, b0, na, nb, shape))
                adj, cum, at = [], [], 0
                for r in range(4):
                    off = c.put(four[at:at + counts[r]])
                    adj.append(off - kb * at)
                    cum.append(at)
                    at += counts[r]
                off1 = c.put(one)
                if kind == "14":
                    c.set_A([off1], [0], len(one)); c.set_B(adj, cum, len(four))
                else:
                    c.set_A(adj, cum, len(four)); c.set_B([off1], [0], len(one))
                out = c.room(kb * (na + nb))
                c.desc[D_OUT] = out
                c.p(which, a0, b0, na, nb)
                sa, sb_ = first[a0:a0 + na], second[b0:b0 + nb]
                c.want(out, ln.merge128(sa, sb_) if wide else np.concatenate([sa, sb_]))
                cases.append(c)
    run_cases(L, LK_TILE, cases)


# ================================================== repairs ==================================================
RUN_LENGTHS = (0, 1, 2, 63, 64, 65, 128, 129, 200)


def repair_runs(rng, n):
    """-> [(placement, run)]: ascending runs of n even keys with misfits (odd keys) put in by hand"""
    base = np.sort(distinct_keys(rng, n, hi=1 << 40)) + U64(1 << 20)

    def misfit_at(run, *idx):       # run[i] becomes a key smaller than its predecessor (odd, so distinct from every other key)
        run = run.copy()
        for j, i in enumerate(idx):
            run[i] = base[0] - U64(1 + 2 * j) if i < 2 else base[i - 2] + U64(1)
        return run

    out = [("no misfit", base)]
    if n >= 2:
        out.append(("last valid lane", misfit_at(base, n - 1)))
        out.append(("second key", misfit_at(base, 1)))
        d = base[::-1].copy()
        out.append(("descending", d))
        e = base.copy()
        e[0] = U64(1 << 62)         # an early large key: every later key is a misfit
        out.append(("first key largest", e))
        t = base.copy()
        t[n // 2] = t[n // 2 - 1] if n // 2 >= 1 else t[0]        # equal neighbours: kept (k < pk is strict) -- ties are legal here
        out.append(("equal neighbours", t))
    if n >= 5:                      # ... and with a misfit in the same chunk, which sends the chunk through the exact running maximum
        t = base.copy()
        t[n // 2] = t[n // 2 - 1]
        out.append(("equal neighbours and a misfit", misfit_at(t, n // 2 + 2)))
    if n >= 3:
        e = base.copy()
        e[1] = U64(1 << 62)
        out.append(("second key largest", e))
        z = base.copy()             # smaller than the running maximum but not than its neighbour: only the exact maximum sees it
        z[n // 3] = U64(1 << 61)
        out.append(("large key at a third", z))
    if n > 64:
        out.append(("lane 0 of chunk 1", misfit_at(base, 64)))
        out.append(("chunk 0 only, clean chunks behind", misfit_at(base, 5)))
        out.append(("chunk 0 twice, clean chunks behind", misfit_at(base, 5, 40)))
        out.append(("last lane of chunk 0", misfit_at(base, 63)))
    if n > 128:
        out.append(("consecutive chunks", misfit_at(base, 10, 70, 128)))
        out.append(("lane 0 of chunks 1 and 2", misfit_at(base, 64, 128)))
        t = base.copy()
        t[64] = t[63]               # equal neighbours across a chunk boundary: the carry decides, and keeps it
        out.append(("equal neighbours across chunks", t))
    return out


def widen(rng, run, mode):
    """a run of narrow keys as 128-bit keys in the same order"""
    if mode == "a":                 # a decides, b arbitrary
        return np.stack([run, rng.integers(0, ln.M64, size=len(run), dtype=np.uint64)], axis=1)
    return np.stack([np.full(len(run), 77 << 30, dtype=U64), run], axis=1)      # all tie on a: b decides


def repair_expect(c, run_off, run, kb, lt=None):
    """the expectation of one run's repair, into case c: kept keys in order, the run's tail free, misfits a multiset behind the first nx0 keys.
    -> (number of misfits, their keys)"""
    rows = [tuple(int(v) for v in np.atleast_1d(k)) for k in run] if kb == 16 else [int(k) for k in run]
    kept, mis = ln.repair(rows, lt)
    if kept:
        c.want(run_off, run[kept])
    if mis:
        c.free.append((run_off + kb * len(kept), kb * len(mis)))
    return len(mis), run[mis]


def check_repair_run(L, wide):
    rng = np.random.default_rng(61 + wide)
    kb = 16 if wide else 8
    lt = ln.wk_lt if wide else None
    cases = []
    for n in RUN_LENGTHS:
        for nx0 in (0, 37):
            for mode in (("a", "b") if wide else ("",)):
                for place, run in repair_runs(rng, n):
                    if wide:
                        run = widen(rng, run, mode)
                    if "equal" not in place:
                        (check_keys128 if wide else check_keys)(run)
                    c = Case("repair%s_run n=%d nx=%d %s %s" % ("w" if wide else "", n, nx0, place, mode))
                    run_off = c.put(run)
                    nm, mk = repair_expect(c, run_off, run, kb, lt)
                    xk = distinct_keys(rng, nx0, hi=1 << 19)
                    xk = np.stack([xk, xk], axis=1) if wide else xk
                    # the keys that were there, and exactly the misfits' room behind them
                    x_off = c.put(np.concatenate([xk.reshape(-1).view(U8), np.full(kb * nm, BG, dtype=U8)]))
                    c.free.append((x_off + kb * nx0, kb * nm))
                    c.set_A([run_off], [0], n)
                    c.desc[D_OUT] = x_off
                    c.p(nx0, 1 if wide else 0)
                    c.want_ret = nm

                    def post(d, slot, x_off=x_off, nx0=nx0, nm=nm, mk=mk, name=c.name):
                        got = slot[x_off + kb * nx0:x_off + kb * (nx0 + nm)].view(U64).reshape(nm, kb // 8)
                        want = np.asarray(mk, dtype=U64).reshape(nm, kb // 8)
                        assert sorted(map(tuple, got.tolist())) == sorted(map(tuple, want.tolist())), name + ": misfits"
                    c.post = post
                    cases.append(c)
    run_cases(L, LK_REPAIR_RUN, cases)


def check_repair_runs4(L):
    rng = np.random.default_rng(64)
    cases = []
    cap = 640                      # keys per run area (max_paths): room for every run's misfits behind the unsorted run's keys
    run_bytes = 8 * cap
    length_sets = [(200, 65, 1, 0), (64, 128, 129, 2), (130, 130, 130, 130), (0, 0, 0, 5), (1, 1, 1, 1), (0, 1, 200, 63), (129, 0, 2, 1), (2, 2, 2, 2)]
    for lens in length_sets:
        per_run = [repair_runs(rng, n) for n in lens]
        nvar = max(len(p) for p in per_run)
        for var in range(nvar):
            for nx0 in (0, 37):
                runs = [p[(var + 3 * r) % len(p)] for r, p in enumerate(per_run)]
                # the four runs hold distinct keys between them too: run r's keys get r in bits 44..45
                keys = [(run + (U64(r) << U64(44))) if len(run) else run for r, (_, run) in enumerate(runs)]
                check_keys(np.concatenate([np.unique(k) for k in keys]))
                c = Case("repair_runs4 lens=%s nx=%d [%s]" % (lens, nx0, " | ".join(p for p, _ in runs)))
                stays = distinct_keys(rng, 9, hi=1 << 19)
                area = np.full(6 * run_bytes, BG, dtype=U8)
                area[:72] = stays.view(U8)
                for r in range(4):
                    area[(r + 1) * run_bytes:(r + 1) * run_bytes + 8 * lens[r]] = keys[r].view(U8)
                xk = distinct_keys(rng, nx0, hi=1 << 19) + U64(1 << 50)
                area[5 * run_bytes:5 * run_bytes + 8 * nx0] = xk.view(U8)
                str_off = c.put(area)
                x_off = str_off + 5 * run_bytes
                counts, allmis = [], []
                for r in range(4):
                    if lens[r] > 1:
                        nm, mk = repair_expect(c, str_off + (r + 1) * run_bytes, keys[r], 8)
                    else:
                        nm, mk = 0, keys[r][:0]         # (a run of one key, or none, is not touched: its area stays as it is)
                    counts.append(nm)
                    allmis.append(mk)
                allmis = np.concatenate(allmis)
                assert nx0 + len(allmis) <= cap
                c.free.append((x_off + 8 * nx0, 8 * len(allmis)))
                c.desc[D_AADJ] = str_off
                c.desc[D_ACUM:D_ACUM + 4] = lens
                c.desc[D_OUT] = x_off
                c.p(nx0, run_bytes)
                c.want_ret = counts[0] | counts[1] << 16 | counts[2] << 32 | counts[3] << 48

                def post(d, slot, x_off=x_off, nx0=nx0, allmis=allmis, name=c.name):
                    got = slot[x_off + 8 * nx0:x_off + 8 * (nx0 + len(allmis))].view(U64)
                    assert np.array_equal(np.sort(got), np.sort(allmis)), name + ": a misfit lost or duplicated"
                c.post = post
                cases.append(c)
    run_cases(L, LK_REPAIR_RUNS4, cases)




# ================================================== the chain of phase S ==================================================
def chain_runs(rng, lens, nmis, wide):
    """-> (stays, [four runs of moves], unsorted): the moves ascending across their runs but for nmis inversions inside runs"""
    nm = sum(lens[1:5])
    if wide:        # many keys tie on a; b (distinct) decides.  The unsorted run's b have bit 63 set, the others' do not
        mk = ln.sort128(np.stack([rng.integers(1, 40, size=nm, dtype=np.uint64) << U64(31), distinct_keys(rng, nm, hi=1 << 63)], axis=1))
        xk = np.stack([rng.integers(1, 40, size=lens[5], dtype=np.uint64) << U64(31), distinct_keys(rng, lens[5], hi=1 << 63) | U64(1 << 63)], axis=1)
        st = np.sort(distinct_keys(rng, lens[0], hi=1 << 19))
        stays = np.stack([st, st], axis=1)
    else:           # moves even, the unsorted run's keys odd
        mk = np.sort(distinct_keys(rng, nm, hi=1 << 40)) + U64(1 << 20)
        xk = distinct_keys(rng, lens[5], hi=1 << 40) + U64((1 << 20) + 1)
        stays = np.sort(distinct_keys(rng, lens[0], hi=1 << 19))
    runs, at = [], 0
    for r in range(1, 5):
        runs.append(mk[at:at + lens[r]].copy())
        at += lens[r]
    live = [r for r in range(4) if lens[r + 1] > 2]
    for j in range(nmis):       # nested parents: two neighbours of a run change places, the second is then smaller than the first
        r = live[j % len(live)]
        i = int(rng.integers(1, len(runs[r])))
        runs[r][[i - 1, i]] = runs[r][[i, i - 1]]
    return stays, runs, xk


def check_chain(L, wide):
    """six runs as phase E files them -> repair -> sort of the unsorted run -> merge with the moves, in phase_S's offsets and KeyArrs.  The merged
    moves-and-unsorted sequence against a plain sort; the stays and everything between the areas unchanged"""
    rng = np.random.default_rng(70 + wide)
    kb = 16 if wide else 8
    lt = ln.wk_lt if wide else None
    cases = []
    for lens, nmis in (((60, 50, 50, 50, 47, 20), 3), ((300, 240, 230, 250, 200, 80), 9), ((10, 120, 1, 0, 130, 1), 2), ((5, 100, 90, 80, 70, 0), 0),
                       ((5, 100, 90, 80, 70, 0), 4), ((0, 200, 210, 190, 180, 520), 6)):
        assert sum(lens) > MERGE_MIN
        cap = max(lens) + nmis + 16             # keys per run area (max_paths)
        run_bytes = kb * cap
        stays, runs, xk = chain_runs(rng, lens, nmis, wide)
        allk = np.concatenate(runs + [xk])
        (check_keys128 if wide else check_keys)(allk)
        c = Case("chain %s lens=%s inversions=%d" % ("wide" if wide else "narrow", lens, nmis))
        area = np.full(6 * run_bytes, BG, dtype=U8)
        area[:kb * lens[0]] = stays.reshape(-1).view(U8)
        for r in range(4):
            area[(r + 1) * run_bytes:(r + 1) * run_bytes + kb * lens[r + 1]] = runs[r].reshape(-1).view(U8)
        area[5 * run_bytes:5 * run_bytes + kb * lens[5]] = xk.reshape(-1).view(U8)
        str_off = c.put(area)
        x_off = str_off + 5 * run_bytes
        kept_counts, nxe = [], lens[5]
        for r in range(4):
            if lens[r + 1] > 1:
                nm, _ = repair_expect(c, str_off + (r + 1) * run_bytes, runs[r], kb, lt)
            else:
                nm = 0
            kept_counts.append(lens[r + 1] - nm)
            nxe += nm
        assert nxe <= cap and (nmis == 0 or nxe > lens[5])
        c.free.append((x_off, kb * nxe))        # the unsorted run: sorted in place (narrow), left as repaired (wide)
        skeys = 0
        if wide:
            room = nxe if nxe <= 512 else 1024  # (the legacy network pads to a power of two of at least 1024 keys)
            skeys = c.room(16 * room)
            c.free.append((skeys, 16 * room))
        km, total = sum(kept_counts), sum(lens[1:])
        out = c.room(kb * total)
        c.desc[D_AADJ] = str_off
        c.desc[D_ACUM:D_ACUM + 4] = lens[1:5]
        c.desc[D_OUT] = out
        c.p(lens[5], run_bytes, skeys, 1 if wide else 0)
        merged = ln.sort128(allk) if wide else ln.sort64(allk)
        assert km > 0
        if nxe > 0:
            c.want(out, merged)
            c.want_ret = total | out << 32
        else:                                   # nothing to merge: KB names the moves where they lie
            assert np.array_equal(np.concatenate(runs), merged)
            c.want_ret = km | (str_off + run_bytes) << 32

        def post(d, slot, kept_counts=kept_counts, name=c.name):
            assert [int(d[D_P + 4]), int(d[D_P + 5]), int(d[D_P + 6]), int(d[D_AN])] == kept_counts, name + ": counts after the repair"
        c.post = post
        cases.append(c)
    run_cases(L, LK_CHAIN, cases)
