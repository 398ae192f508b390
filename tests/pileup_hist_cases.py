"""The cases of the pile-up's level histograms and of the Kolmogorov-Smirnov kernel (k_pileup_hist.hip, unc_pileup_hist.cpp, the add
in k_pileup.hip), shared by tests/test_pileup_hist_cpu.py (the lanesim emulator) and tests/test_gpu_pileup_hist.py (the MI355X).  X and
M are the contexts of tests/pileup_cases.py (the bundled example, the five-sequence reference); the independent checker is
tests/pileup_hist_naive.py (Python integers and fractions) beside tests/pileup_naive.py.

The shapes: k_pileup_accum takes 1024 records a workgroup, so 3 * 1024 + 100 records are four workgroups; k_pileup_hist_centres takes
256 positions a workgroup; k_pileup_ks takes a bin a wavefront, four a workgroup, so 257 listed bins are 65 workgroups, the last with
one wavefront at work.  Everything is exact: there is no tolerance anywhere, doubles are compared as their 64 bits."""
import ctypes as C

import numpy as np

import model_cases as mc
import pileup_cases as pc
import pileup_hist_naive as hn
import pileup_naive as pn

ERR_ARG = -1
W_DEFAULT = 0.25
BUCKETS = 64


def all_bins(pu):
    return np.arange(pu.n_bins(), dtype=np.uint64)


def pairs_of(X, model):
    from uncalled_amd import capi
    return (model if model is not None else capi.Model.default(lib=X.L)).pairs()


def centres_by_stats(pu, pairs, bins=None):
    """what the issue states: llrint(pairs[stats(bin).kmer].mean * 2^20)"""
    bins = all_bins(pu) if bins is None else bins
    return [hn.centre_of(pairs[int(k), 0]) for k in pu.stats(bins)["kmer"]]


def naive_for(pu, regions, pairs, width, keep_shared=False):
    """the naive histograms of a pile-up over `regions` (small ones: every bin's centre is looked up at once)"""
    keys = pn.Naive(regions).keys_in_order()
    centre = dict(zip(keys, centres_by_stats(pu, pairs)))
    return hn.Hist(regions, centre.__getitem__, hn.width_of(width), keep_shared)


def equals_naive(pu, nh):
    """the table as in pileup_cases, every bin's 64 buckets, and the invariant: a bin's buckets sum to its n"""
    got = pc.equals_naive(pu, nh.nv)
    rows = pu.hist(all_bins(pu))
    assert rows.shape == (pu.n_bins(), BUCKETS) and rows.dtype == np.uint32
    keys = nh.nv.keys_in_order()
    bad = [(i, k) for i, k in enumerate(keys) if rows[i].tolist() != nh.row(k)]
    assert not bad, (bad[:3], [rows[i].tolist() for i, _ in bad[:3]], [nh.row(k) for _, k in bad[:3]])
    assert np.array_equal(rows.sum(axis=1, dtype=np.uint64), got["n"])
    return rows


def both(pu, nh, *rec):
    pu.add(*rec)
    nh.add(*rec)


def state(pu):
    return pc.table(pu).tobytes(), pu.hist(all_bins(pu)).tobytes(), pu.counters()


# ------------------------------------------------------------------ 1. centres
def case_centres(X):
    """1. a 60-base region of the example, both strands, the r9.4 template and a random model: every bin's centre is the fixed-point
    mean of the k-mer stats reports, which is ref_kmers' of the same place.  A pile-up without a histogram has no centres"""
    from uncalled_amd import capi
    regions = [(0, 4000, 4060)]
    custom = capi.Model.from_pairs(mc.random_pairs(31), lib=X.L)
    for model in (None, custom):
        pairs = pairs_of(X, model)
        pu = X.pileup(regions)
        before = pu.device_bytes()
        pu.enable_hist(W_DEFAULT, model)
        assert pu.n_bins() == 112 and pu.device_bytes() == before + 112 * (BUCKETS * 4 + 8)
        got = pu.hist_centres(all_bins(pu))
        assert got.dtype == np.int64 and got.tolist() == centres_by_stats(pu, pairs)
        kms = [int(capi.ref_kmers(X.index, X.prefix, 0, 4000 + b // 2, 4005 + b // 2, b % 2 == 0)[0]) for b in range(112)]
        assert got.tolist() == [hn.centre_of(pairs[k, 0]) for k in kms] and len(set(kms)) > 50
        assert not pu.hist(all_bins(pu)).any()
    plain = X.pileup(regions)
    out = np.zeros(1, np.int64)
    assert X.L.unc_pileup_hist_centres(plain.h, 1, np.zeros(1, np.uint64).ctypes.data, out.ctypes.data) == ERR_ARG
    rows = np.zeros(BUCKETS, np.uint32)
    assert X.L.unc_pileup_hist_gather(plain.h, 1, np.zeros(1, np.uint64).ctypes.data, rows.ctypes.data) == ERR_ARG and not rows.any()


def case_centres_sequences(M):
    """1, continued: five sequences.  Regions at both ends of every sequence that holds a bin, two that touch inside sequence 2, one of
    four bases; the first and last bin of each sequence and the bins either side of the region edges get the k-mer of the FASTA string
    there, which is stats', on both strands: an offset without its sequence, or a region's first base taken for another's, would
    show.  More than 256 positions, so k_pileup_hist_centres runs several workgroups"""
    from uncalled_amd import capi
    n = M.lens
    regions = [(4, n[4] - 300, n[4]), (2, 300, 600), (0, 0, n[0]), (2, 0, 300), (3, 0, n[3]), (2, n[2] - 200, n[2]), (4, 0, 300), (1, 0, 4)]
    custom = capi.Model.from_pairs(mc.random_pairs(32), lib=M.L)
    for model in (None, custom):
        pairs = pairs_of(M, model)
        pu = M.pileup(regions)
        pu.enable_hist(W_DEFAULT, model)
        nv = pn.Naive(regions)
        keys = nv.keys_in_order()
        assert pu.n_bins() == len(keys) == 2 * (137 + 296 + 296 + 196 + 146 + 296 + 296) and pu.n_bins() // 2 > 4 * 256
        got = pu.hist_centres(all_bins(pu)).tolist()
        want = [hn.centre_of(pairs[pn.py_kmer(M.seqs[r], p, s == 0), 0]) for r, p, s in keys]
        bad = [(i, keys[i]) for i in range(len(keys)) if got[i] != want[i]]
        assert not bad, (len(bad), bad[:4])
        assert got == centres_by_stats(pu, pairs)
        edges = [(r, p, s) for r in (0, 2, 3, 4) for p in (0, n[r] - 5) for s in (0, 1)] + [(2, p, s) for p in (295, 300, 595) for s in (0, 1)]
        listed = np.array([nv.bin_of(k) for k in edges][::-1], np.uint64)      # a list in no order
        assert pu.hist_centres(listed).tolist() == [want[int(b)] for b in listed]


# ------------------------------------------------------------------ 2. bucket edges
def small_model(X, seed):
    """means in -4 .. 4: every integer q near a centre is a float32 level (24 significant bits), which no model of real levels allows"""
    from uncalled_amd import capi
    rng = np.random.default_rng(seed)
    pairs = np.stack([rng.uniform(-4, 4, 1024), np.ones(1024)], axis=1).astype(np.float32)
    return capi.Model.from_pairs(pairs, lib=X.L)


def case_bucket_edges(X):
    """2. w = 1, w = llrint(0.25 * 2^20) and w = 2^31; records at the model's mean as a float (q == c: bucket 32), at its two float
    neighbours, at +-2047.99, and at q - c = k w - 1 and k w for the bucket edges k = -32, -31, 0, 1, 31, 32 -- for w = 1 these are
    q - c = -33, -32, -1, 0, 31, 32 among others.  The levels are searched for (a float32 with exactly that q) and must be found.  Both
    strands, a model of small means and, for the width of 0.25, the r9.4 template"""
    regions = [(0, 4000, 4060)]
    for width, w, model in ((2.0 ** -20, 1, small_model(X, 33)), (W_DEFAULT, 1 << 18, small_model(X, 34)), (2048.0, 1 << 31, small_model(X, 35)),
                            (W_DEFAULT, 1 << 18, None)):
        assert hn.width_of(width) == w
        pairs = pairs_of(X, model)
        pu = X.pileup(regions)
        pu.enable_hist(width, model)
        nh = naive_for(pu, regions, pairs, width)
        assert nh.w == w
        for key in ((0, 4010, 0), (0, 4033, 1)):
            c = nh.centre(key)
            mean = np.float32(pu.stats([nh.nv.bin_of(key)], model)["model_mean"][0])
            assert pn.q_of(mean) == c
            levels = [mean, np.nextafter(mean, np.float32(np.inf)), np.nextafter(mean, np.float32(-np.inf)), np.float32(2047.99), np.float32(-2047.99)]
            deltas = sorted({k * w - d for k in (-32, -31, 0, 1, 31, 32) for d in (1, 0)} | ({-33, -32, -1, 0, 31, 32} if w == 1 else set()))
            reach = 2 ** 24 if model is not None else 2047 * pn.ONE         # every integer below 2^24 is a float32
            found = {d: hn.level_with_q(c + d) for d in deltas if abs(c + d) < reach}
            if model is not None:
                assert all(lv is not None for lv in found.values()), [d for d, lv in found.items() if lv is None]
                assert w == 1 << 31 or len(found) == len(deltas)
            levels += [lv for lv in found.values() if lv is not None]
            m = len(levels)
            both(pu, nh, np.full(m, key[0], np.int32), np.full(m, key[1]), np.full(m, 1 - key[2]), np.array(levels, np.float32), np.ones(m, np.uint32))
            row = nh.row(key)
            assert sum(row) == m and row[32] >= 1 and hn.bucket_of(c, c, w) == 32
            if w == 1:
                assert [hn.bucket_of(c + d, c, 1) for d in (-33, -32, -1, 0, 31, 32)] == [0, 0, 31, 32, 63, 63]
                assert row[0] >= 3 and row[63] >= 3 and row[31] >= 1
            if w == 1 << 31:          # t / w = 32 + floor((q - c) / 2^31), and |q - c| < 2^31 + 2^23
                assert {31, 32} <= {i for i, x in enumerate(row) if x} <= {30, 31, 32, 33}
        rows = equals_naive(pu, nh)
        assert int(rows.sum()) == pu.counters()[2] >= 14


# ------------------------------------------------------------------ 3. one bin, many workgroups
def numpy_row(levels, c, w):
    q = np.rint(np.asarray(levels, np.float32).astype(np.float64) * pn.ONE).astype(np.int64)
    return np.bincount(np.clip((q - c + 32 * w) // w, 0, BUCKETS - 1), minlength=BUCKETS)


def case_one_bin(X):
    """3. 3 * 1024 + 100 records, four workgroups of k_pileup_accum, at one bin, on either strand: the histogram equals numpy's and
    sums to n.  Then case 3 of the pile-up with a histogram: dropped, outside and shared records add to no bucket, and
    UNC_PILEUP_KEEP_SHARED adds the shared ones"""
    rng = np.random.default_rng(3)
    n = 3 * pc.RECS_PER_BLOCK + 100
    regions = [(0, 500, 600)]
    pairs = pairs_of(X, None)
    w = hn.width_of(W_DEFAULT)
    for fwd in (1, 0):
        pu = X.pileup(regions)
        pu.enable_hist(W_DEFAULT)
        bin_ = 2 * 37 + (0 if fwd else 1)
        c = centres_by_stats(pu, pairs, np.array([bin_], np.uint64))[0]
        lv = rng.normal(c / pn.ONE, 3.0, n).astype(np.float32)
        pu.add(np.zeros(n, np.int32), np.full(n, 537), np.full(n, fwd), lv, rng.integers(1, 40, n))
        rows = pu.hist(all_bins(pu))
        want = numpy_row(lv, c, w)
        assert rows[bin_].tolist() == want.tolist() and int(rows[bin_].sum()) == n == int(pu.gather([bin_])["n"][0])
        assert int(rows.sum()) == n and want[0] > 0 and want[63] > 0 and (want > 0).sum() > 50
    regions = [(0, 700, 760)]
    lv = np.array([np.nan, np.inf, -np.inf, 2048.0, -2048.0, 2047.99, 80.0, 90.0, 70.0, 71.0, 72.0, 73.0], np.float32)
    pos = np.array([710, 711, 712, 713, 714, 715, 716, 716, 756, 699, 700, 755])
    sh = np.array([0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0], np.uint32)
    for keep in (False, True):
        pu = X.pileup(regions, keep)
        pu.enable_hist(W_DEFAULT)
        nh = naive_for(pu, regions, pairs, W_DEFAULT, keep)
        both(pu, nh, np.zeros(12, np.int32), pos, np.ones(12), lv, np.full(12, 9), sh)
        rows = equals_naive(pu, nh)
        assert pu.counters() == (5, 2, 5 if keep else 4) and int(rows.sum()) == (5 if keep else 4) and int(rows[2 * 16].sum()) == (2 if keep else 1)


# ------------------------------------------------------------------ 4. order, split, reset, merge, what enable refuses
def case_order_split_reset(X):
    """4. the same 5 000 records in one call and shuffled in three: identical bytes, equal to the naive histograms; reset zeroes the
    buckets, keeps the histogram attached with its centres, and adding again reproduces them"""
    rng = np.random.default_rng(4)
    regions = [(0, 1000, 1104)]
    pairs = pairs_of(X, None)
    rec = list(pc.random_records(rng, 5000, 990, 1110))
    rec[3] = (90 + rng.standard_normal(5000) * 6).astype(np.float32)
    rec[3][::97] = np.inf
    one, three = X.pileup(regions), X.pileup(regions)
    one.enable_hist(W_DEFAULT)
    three.enable_hist(W_DEFAULT)
    nh = naive_for(one, regions, pairs, W_DEFAULT)
    both(one, nh, *rec)
    for part in np.array_split(rng.permutation(5000), 3):
        three.add(*[a[part] for a in rec])
    assert state(one) == state(three)
    rows = equals_naive(one, nh)
    assert nh.nv.dropped > 0 and nh.nv.outside > 0 and nh.nv.added > 3000 and (rows > 0).sum() > 1000
    first, centres, size = state(one), one.hist_centres(all_bins(one)).tobytes(), one.device_bytes()
    one.reset()
    assert not one.hist(all_bins(one)).any() and not pc.table(one).view(np.uint64).any() and one.counters() == (0, 0, 0)
    assert one.hist_centres(all_bins(one)).tobytes() == centres and one.device_bytes() == size
    one.add(*rec)
    assert state(one) == first
    return one


def case_merge(X):
    """4, continued: A.merge(B) equals one object fed both sets, buckets included.  Refused, with both tables keeping their bytes: a
    histogram against none (either way round), another width, another model"""
    from uncalled_amd import capi
    rng = np.random.default_rng(41)
    regions = [(0, 3000, 3100), (0, 3300, 3310)]
    pairs = pairs_of(X, None)

    def records(n):
        rec = list(pc.random_records(rng, n, 2990, 3320))
        rec[3] = (95 + rng.standard_normal(n) * 8).astype(np.float32)
        return rec
    one, two = records(3000), records(2000)
    A, B, Cc = X.pileup(regions), X.pileup(regions), X.pileup(regions)
    for pu in (A, B, Cc):
        pu.enable_hist(W_DEFAULT)
    nh = naive_for(Cc, regions, pairs, W_DEFAULT)
    A.add(*one)
    B.add(*two)
    both(Cc, nh, *one)
    both(Cc, nh, *two)
    A.merge(B)
    assert state(A) == state(Cc)
    equals_naive(A, nh)
    plain, wide, other = X.pileup(regions), X.pileup(regions), X.pileup(regions)
    wide.enable_hist(0.5)
    other.enable_hist(W_DEFAULT, capi.Model.from_pairs(mc.random_pairs(42), lib=X.L))
    same = X.pileup(regions)
    same.enable_hist(W_DEFAULT, capi.Model.default(lib=X.L))          # the template given as an object is the template
    for pu in (plain, wide, other, same):
        pu.add(*two)
    kept = {id(pu): (pc.table(pu).tobytes(), pu.counters()) for pu in (plain, wide, other)}
    mine = state(A)
    for pu in (plain, wide, other):
        for dst, src in ((A, pu), (pu, A)):
            assert X.L.unc_pileup_merge(dst.h, src.h) == ERR_ARG and X.L.unc_last_error()
        assert (pc.table(pu).tobytes(), pu.counters()) == kept[id(pu)] and state(A) == mine
    A.merge(same)
    for r in (two,):
        both(Cc, nh, *r)
    assert state(A) == state(Cc)


def case_enable_refusals(X):
    """4, continued: unc_pileup_hist_enable refuses a pile-up that holds records (added, dropped or outside ones), a second histogram,
    a width whose w is not in 1 .. 2^31 or that is not finite, and a model with a mean of 2048 or more; the pile-up is then as it was
    and takes a histogram afterwards"""
    from uncalled_amd import capi
    regions = [(0, 100, 200)]
    one = (np.zeros(1, np.int32), np.array([150]), np.ones(1), np.array([80], np.float32), np.ones(1))
    for rec in (one, one[:3] + (np.array([np.inf], np.float32),) + one[4:], one[:1] + (np.array([300]),) + one[2:]):
        pu = X.pileup(regions)
        pu.add(*rec)
        assert sum(pu.counters()) == 1
        assert X.L.unc_pileup_hist_enable(pu.h, None, C.c_float(W_DEFAULT)) == ERR_ARG and b"records" in X.L.unc_last_error()
        pu.reset()
        pu.enable_hist(W_DEFAULT)
    pu = X.pileup(regions)
    size = pu.device_bytes()
    for width in (0.0, -0.25, 2.0 ** -22, 2048.5, 1e30, np.inf, -np.inf, np.nan):
        assert X.L.unc_pileup_hist_enable(pu.h, None, C.c_float(width)) == ERR_ARG, width
    bad = mc.random_pairs(43)
    for mean in (2048.0, -2048.0, 3e38):
        bad[1023, 0] = mean
        model = capi.Model.from_pairs(bad, lib=X.L)
        assert X.L.unc_pileup_hist_enable(pu.h, model.h, C.c_float(W_DEFAULT)) == ERR_ARG and b"mean" in X.L.unc_last_error(), mean
    assert pu.device_bytes() == size
    bad[1023, 0] = -2047.99
    pu.enable_hist(2048.0, capi.Model.from_pairs(bad, lib=X.L))
    assert pu.device_bytes() == size + pu.n_bins() * (BUCKETS * 4 + 8)
    assert X.L.unc_pileup_hist_enable(pu.h, None, C.c_float(W_DEFAULT)) == ERR_ARG and b"already" in X.L.unc_last_error()
    X.pileup(regions).enable_hist(2.0 ** -20)
    empty = X.pileup([(0, 100, 104)])
    empty.enable_hist(W_DEFAULT)
    assert empty.n_bins() == 0 and empty.hist([]).shape == (0, BUCKETS)


# ------------------------------------------------------------------ 5. through the alignment
def case_through_the_alignment(X, R):
    """5. unc_align_pileup_call on pileup_cases' batch with a histogram, in one round and with a workspace that forces three or more:
    table and histogram equal those of array mode fed the call's own segments, and everything the call returns is bit for bit what it
    returns for a pile-up without a histogram, whose table is the same too"""
    from uncalled_amd import capi
    qs, stretches = pc.batch(R)
    kw = dict(levels=True, paths=True, kmers=True, segments=True)
    first = None
    for ws in (0, 6200):
        pu, plain, fed = X.pileup(), X.pileup(), X.pileup()
        pu.enable_hist(W_DEFAULT)
        fed.enable_hist(W_DEFAULT)
        out = capi.align_ref_batch(X.refseq, R.raw, R.offsets, R.calib, qs, stretches, None, workspace_bytes=ws, pileup=pu, **kw)
        res, _, _, _, segs, info = out
        assert (res["status"] == capi.DTW_OK).all() and (info["status"] == capi.SEG_OK).all()
        assert capi.dtw_last_timing(X.L)[1] >= 3 if ws else capi.dtw_last_timing(X.L)[1] == 1
        pc.same_outputs(out, capi.align_ref_batch(X.refseq, R.raw, R.offsets, R.calib, qs, stretches, None, workspace_bytes=ws, pileup=plain, **kw))
        assert pc.table(pu).tobytes() == pc.table(plain).tobytes() and pu.counters() == plain.counters()
        for s, seg, inf in zip(stretches, segs, info):
            rows = int(inf["row_first"]) + np.arange(seg.size)
            fed.add(np.full(seg.size, s[0], np.int32), [pc.row_pos(s, int(r)) for r in rows], np.full(seg.size, 1 if s[3] else 0), seg["level"],
                    seg["smp_n"], seg["shared"])
        cov = pu.covered(1)
        assert pu.counters()[2] > 300 and cov.size > 200
        assert pu.hist(cov).tobytes() == fed.hist(cov).tobytes() and pc.table(pu).tobytes() == pc.table(fed).tobytes()
        rows = pu.hist(cov)
        assert np.array_equal(rows.sum(axis=1, dtype=np.uint64), pu.gather(cov)["n"]) and int(rows.sum()) == pu.counters()[2]
        assert int(fed.hist(all_bins(fed)).sum(dtype=np.uint64)) == pu.counters()[2]
        if first is None:
            first = pu.hist(cov).tobytes()
        assert pu.hist(cov).tobytes() == first           # the rounds do not change the histogram


# ------------------------------------------------------------------ 6. the Kolmogorov-Smirnov kernel against the checker
def fill_buckets(pu, pos, fwd, c, w, buckets):
    """one record in each listed bucket of the bin at (0, pos): a level in the middle of the bucket, which must exist as a float32"""
    levels = [hn.level_with_q(c + (k - 32) * w + w // 2) for k in buckets]
    assert all(lv is not None for lv in levels) and [hn.bucket_of(pn.q_of(lv), c, w) for lv in levels] == list(buckets)
    m = len(levels)
    if m:
        pu.add(np.zeros(m, np.int32), np.full(m, pos), np.full(m, fwd), np.array(levels, np.float32), np.ones(m, np.uint32))


def check_ks(got, rows_a, rows_b):
    from uncalled_amd import capi
    assert got.dtype == capi.PILEUP_KS and len(got) == len(rows_a) == len(rows_b)
    for i, (ra, rb) in enumerate(zip(rows_a, rows_b)):
        n_a, n_b, num, bucket, sign, d, ks = hn.ks([int(x) for x in ra], [int(x) for x in rb])
        g = got[i]
        assert (int(g["n_a"]), int(g["n_b"]), int(g["num"]), int(g["bucket"]), int(g["sign"])) == (n_a, n_b, num, bucket, sign), (i, g)
        assert [int(x) for x in pn.bits([g["d"], g["ks"]])] == [int(x) for x in pn.bits([d, ks])], (i, g, d, ks)


def mid_model(X, seed):
    """means in 70 .. 110: the centres are multiples of 8 and every bucket's middle lies below 128 levels, so it is a float32 level"""
    from uncalled_amd import capi
    rng = np.random.default_rng(seed)
    return capi.Model.from_pairs(np.stack([rng.uniform(70, 110, 1024), rng.uniform(1, 3, 1024)], axis=1).astype(np.float32), lib=X.L)


def case_ks(X, on_gpu=False):
    """6. pairs of samples built bucket by bucket at positions 4000 .. of a region, plus strand and some on the minus strand: equal
    samples (num 0, sign 0, bucket 0); disjoint ones either way round (num = n_a n_b, d = 1, both signs); two buckets that tie for the
    maximum (the lower is reported); n_a != n_b; one record a side, in one bucket and in two; the end buckets; random rows.  Every
    field equals the checker's, the doubles bit for bit.  Then a list of 257 bins with duplicates, in no order (65 workgroups, the last
    partly full), and a.ks(a)"""
    rng = np.random.default_rng(6)
    regions = [(0, 4000, 4104)]
    model = mid_model(X, 61)
    pairs = pairs_of(X, model)
    w = hn.width_of(W_DEFAULT)
    a, b = X.pileup(regions), X.pileup(regions)
    a.enable_hist(W_DEFAULT, model)
    b.enable_hist(W_DEFAULT, model)
    centres = centres_by_stats(a, pairs)
    hand = [([10, 20, 20, 33], [10, 20, 20, 33]),               # equal
            ([10] * 5, [40] * 7),                               # disjoint, a below b: +1
            ([50] * 3, [2] * 4),                                # disjoint, a above b: -1
            ([10, 20], [15, 15]),                               # +1/2 at 10, -1/2 at 15: a tie, the lower bucket
            ([15, 15], [10, 20]),                               # the same with the signs turned
            ([5] * 9 + [30] * 4, [5, 30, 31]),                  # n_a != n_b
            ([5], [5]), ([5], [6]), ([63], [0]),                # one record a side
            ([0, 63], [0, 0, 63]), (list(range(64)), list(range(0, 64, 2))),
            ([31] * 1000 + [32] * 1001, [31] * 1001 + [32] * 1000)]
    want = []
    for i, (ba, bb) in enumerate(hand):
        pos, fwd = 4000 + i, 1 if i % 3 else 0
        bin_ = 2 * i + (0 if fwd else 1)
        for pu, bk in ((a, ba), (b, bb)):
            fill_buckets(pu, pos, fwd, centres[bin_], w, bk)
        want.append((bin_, np.bincount(ba, minlength=BUCKETS), np.bincount(bb, minlength=BUCKETS)))
    for i in range(len(hand), 100):                             # random rows, 1 .. 40 records a side
        bin_ = 2 * i + int(rng.integers(0, 2))
        ba, bb = (np.clip(np.rint(rng.normal(32 + s, 6, int(rng.integers(1, 41)))), 0, 63).astype(int).tolist() for s in (0, rng.integers(-4, 5)))
        for pu, bk in ((a, ba), (b, bb)):
            fill_buckets(pu, 4000 + i, 1 - bin_ % 2, centres[bin_], w, bk)
        want.append((bin_, np.bincount(ba, minlength=BUCKETS), np.bincount(bb, minlength=BUCKETS)))
    bins = np.array([x[0] for x in want], np.uint64)
    assert a.hist(bins).tolist() == [x[1].tolist() for x in want] and b.hist(bins).tolist() == [x[2].tolist() for x in want]
    got = a.ks(b, bins)
    check_ks(got, [x[1] for x in want], [x[2] for x in want])
    if on_gpu:
        assert a.ks_last_timing() > 0
    assert (int(got["num"][0]), int(got["sign"][0]), int(got["bucket"][0])) == (0, 0, 0) and got["d"][0] == 0 and got["ks"][0] == 0
    assert (int(got["num"][1]), int(got["sign"][1]), int(got["bucket"][1]), got["d"][1]) == (35, 1, 10, 1.0)
    assert (int(got["num"][2]), int(got["sign"][2]), int(got["bucket"][2]), got["d"][2]) == (12, -1, 2, 1.0)
    assert (int(got["bucket"][3]), int(got["sign"][3]), got["d"][3]) == (10, 1, 0.5) and (int(got["bucket"][4]), int(got["sign"][4])) == (10, -1)
    assert [int(x) for x in got["n_a"][5:9]] == [13, 1, 1, 1] and [int(x) for x in got["n_b"][5:9]] == [3, 1, 1, 1]
    assert [got["d"][i] for i in (6, 7, 8)] == [0.0, 1.0, 1.0] and [int(got["sign"][i]) for i in (6, 7, 8)] == [0, 1, -1]
    assert {int(s) for s in got["sign"]} == {-1, 0, 1}
    turned = b.ks(a, bins)
    assert np.array_equal(turned["num"], got["num"]) and np.array_equal(turned["sign"], -got["sign"]) and np.array_equal(turned["bucket"], got["bucket"])
    listed = np.concatenate([bins, rng.choice(bins, 257 - bins.size)])
    rng.shuffle(listed)
    assert listed.size == 257 and np.unique(listed).size < 257
    rows = {int(x[0]): x for x in want}
    check_ks(a.ks(b, listed), [rows[int(x)][1] for x in listed], [rows[int(x)][2] for x in listed])
    same = a.ks(a, listed)
    assert not same["num"].any() and not same["sign"].any() and not same["bucket"].any() and not same["d"].any() and not same["ks"].any()
    assert np.array_equal(same["n_a"], same["n_b"]) and [int(x) for x in same["n_a"]] == [int(rows[int(x)][1].sum()) for x in listed]


# ------------------------------------------------------------------ 7. 64-bit products and what unc_pileup_ks refuses
FIB_START = (1100, 1010, 990, 996)       # records in the four bins of both pile-ups: 4096


def case_ks_wide_and_refusals(X):
    """7. a region of two positions = four bins, 4096 records in each pile-up, then the alternating merges A += B; B += A: after m of
    them the counts are Fibonacci multiples of the start (F(m + 2), F(m + 1)), about 1.6 times more a merge, and the checker's
    integers follow.  After 31 merges both n of every bin lie between 2^31 and 2^32 (2 178 309 and 3 524 578 times 990 .. 1100): the
    products A(k) n_b need all 64 bits, and n_a n_b of bin 0 is above 2^63.  One merge more and an n is 2^32 or more: refused, like
    an empty bin, a pile-up without a histogram, other regions and a bin past the table, `out` staying zero"""
    from uncalled_amd import capi
    rng = np.random.default_rng(7)
    regions = [(0, 4000, 4006)]
    pairs = pairs_of(X, None)
    w = hn.width_of(W_DEFAULT)
    A, B = X.pileup(regions), X.pileup(regions)
    A.enable_hist(W_DEFAULT)
    B.enable_hist(W_DEFAULT)
    assert A.n_bins() == 4 and sum(FIB_START) == 4096
    centres = centres_by_stats(A, pairs)
    rows = {}
    for pu, shift in ((A, 0.0), (B, 0.7)):
        rec = [np.concatenate(x) for x in zip(*[(np.zeros(n, np.int32), np.full(n, 4000 + b // 2), np.full(n, 1 - b % 2),
                                                  rng.normal(centres[b] / pn.ONE + shift, 2.5, n).astype(np.float32), np.ones(n, np.uint32))
                                                 for b, n in enumerate(FIB_START)])]
        pu.add(*rec)
        rows[id(pu)] = [[int(x) for x in numpy_row(rec[3][2 * (rec[1] - 4000) + 1 - rec[2] == b], centres[b], w)] for b in range(4)]
        assert pu.hist(all_bins(pu)).tolist() == rows[id(pu)]
    bins = all_bins(A)
    dst, src = A, B
    for m in range(31):
        dst.merge(src)
        rows[id(dst)] = [[x + y for x, y in zip(ra, rb)] for ra, rb in zip(rows[id(dst)], rows[id(src)])]
        dst, src = src, dst
    # (dst is the one the next merge would go into: the smaller)
    n_small, n_big = [sum(r) for r in rows[id(dst)]], [sum(r) for r in rows[id(src)]]
    assert n_small == [2178309 * s for s in FIB_START] and n_big == [3524578 * s for s in FIB_START]
    assert all(2 ** 31 <= n < 2 ** 32 for n in n_small + n_big)
    assert [int(x) for x in dst.gather(bins)["n"]] == n_small and [int(x) for x in src.gather(bins)["n"]] == n_big
    assert dst.hist(bins).tolist() == rows[id(dst)] and src.hist(bins).tolist() == rows[id(src)]
    assert hn.products(rows[id(A)][0], rows[id(B)][0]) >= 2 ** 63 and all(hn.products(x, y) < 2 ** 64 for x, y in zip(rows[id(A)], rows[id(B)]))
    got = A.ks(B, bins)
    check_ks(got, rows[id(A)], rows[id(B)])
    # (A = p a + q b and B = r a + s b with |p s - q r| = 1: the two large products differ by the start's n times |a(k) - b(k)| only)
    assert got["num"].all() and (got["num"] < np.uint64(2 ** 32)).all() and (got["d"] > 0).all()
    check_ks(B.ks(A, bins[::-1]), rows[id(B)][::-1], rows[id(A)][::-1])

    def refused(a, b, listed):
        listed = np.asarray(listed, np.uint64)
        out = np.zeros(max(1, listed.size), capi.PILEUP_KS)
        rc = X.L.unc_pileup_ks(a.h, b.h, listed.size, listed.ctypes.data, out.ctypes.data)
        return rc == ERR_ARG and bool(X.L.unc_last_error()) and not out.view(np.uint8).any()
    dst.merge(src)
    assert [int(x) for x in dst.gather(bins)["n"]] == [5702887 * s for s in FIB_START] and int(dst.gather(bins)["n"].min()) >= 2 ** 32
    assert refused(A, B, bins) and refused(B, A, bins[:1]) and refused(dst, dst, bins[3:])
    assert not refused(src, src, bins)
    fresh, empty, plain, other = X.pileup(regions), X.pileup(regions), X.pileup(regions), X.pileup([(0, 4000, 4007)])
    for pu in (fresh, empty, other):
        pu.enable_hist(W_DEFAULT)
    for pu in (fresh, plain, other):
        pu.add(np.zeros(4, np.int32), [4000, 4000, 4001, 4001], [1, 0, 1, 0], np.full(4, 90, np.float32), np.ones(4))
    empty.add(np.zeros(3, np.int32), [4000, 4000, 4001], [1, 0, 1], np.full(3, 90, np.float32), np.ones(3))
    assert not refused(fresh, fresh, bins) and not refused(fresh, empty, bins[:3]) and not refused(fresh, src, bins)
    assert refused(fresh, empty, bins) and refused(empty, fresh, [3]) and refused(empty, empty, [0, 3])          # an empty bin
    assert refused(fresh, plain, bins) and refused(plain, fresh, bins) and refused(plain, plain, bins)            # no histogram
    assert refused(fresh, other, bins) and refused(other, fresh, bins)                                            # other regions
    assert refused(fresh, fresh, [0, 4]) and refused(fresh, fresh, [2 ** 63])                                     # a bin past the table
    wide = X.pileup(regions)
    wide.enable_hist(0.5)
    wide.add(np.zeros(4, np.int32), [4000, 4000, 4001, 4001], [1, 0, 1, 0], np.full(4, 90, np.float32), np.ones(4))
    assert refused(fresh, wide, bins)                                                                             # another width


# ------------------------------------------------------------------ 8. layout and symbols
NAMES = ("unc_pileup_hist_enable", "unc_pileup_hist_gather", "unc_pileup_hist_centres", "unc_pileup_ks", "unc_pileup_ks_last_timing")


def case_layout(L):
    """8. the record is 48 bytes, a row 64 * 4; the header declares the new entry points, the library exports them, capi binds them;
    the records that were there keep their sizes"""
    import re
    from pathlib import Path
    from uncalled_amd import capi
    assert capi.PILEUP_KS.itemsize == 48 and capi.PILEUP_HIST_BUCKETS * np.dtype(np.uint32).itemsize == 64 * 4
    assert [capi.PILEUP_KS.fields[f][1] for f in ("n_a", "n_b", "num", "bucket", "sign", "d", "ks")] == [0, 8, 16, 24, 28, 32, 40]
    assert capi.PILEUP_STAT.itemsize == 56 and capi.PILEUP_CMP.itemsize == 64 and capi.PILEUP_WORDS.itemsize == 40 and C.sizeof(capi.AlignCall) == 200
    txt = (Path(__file__).resolve().parents[1] / "include" / "uncalled_hip.h").read_text()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    declared = set(re.findall(r"\b(unc_[a-z0-9_]+)\s*\(", code))
    for name in NAMES:
        assert name in declared and hasattr(L, name) and getattr(L, name).argtypes is not None, name
    assert "unc_pileup_ks_t" in code and "int32_t sign" in code
    for method in ("enable_hist", "hist", "hist_centres", "ks", "ks_last_timing"):
        assert callable(getattr(capi.Pileup, method))
