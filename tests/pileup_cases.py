"""The cases of the signal pile-up (k_pileup.hip, unc_pileup.cpp), shared by tests/test_pileup_cpu.py (the lanesim emulator) and
tests/test_gpu_pileup.py (the MI355X).  X is the context under test: the library (capi.load's handle), the bundled 10 kb example
index and its packed reference.  The independent checker is tests/pileup_naive.py (Python integers, dictionaries keyed
(rid, pos, strand)); the reads are those of tests/segments_cases.py.

The kernels' grid rules (pileup_dev.h), which the shapes below straddle: k_pileup_accum takes 1024 records a workgroup; the
covered-bin kernels take 1024 bins a workgroup, 64 a wavefront's step.  Bins come in strand pairs, so a table's bin count is even:
where a count of bins is named, the cases use the even counts on both sides of it (2, 62, 64, 66, 1022, 1024, 1026, 3074)."""
import ctypes as C

import numpy as np
import pytest

import model_cases as mc
import pileup_naive as pn
import segments_cases as sc

ERR_ARG = -1
RECS_PER_BLOCK = 1024
SCAN_CHUNK = 1024


class Ctx:
    def __init__(self, L, prefix):
        from uncalled_amd import capi
        self.L, self.prefix = L, prefix
        self.index = capi.Index(prefix, lib=L)
        self.refseq = capi.RefSeq(self.index, prefix)
        self.seq_len = int(self.index.seq_len(0))

    def pileup(self, regions=None, keep_shared=False):
        from uncalled_amd import capi
        return capi.Pileup(self.refseq, regions, keep_shared, lib=self.L)


def whole(X):
    return [(0, 0, X.seq_len)]


def table(pu):
    return pu.gather(np.arange(pu.n_bins(), dtype=np.uint64))


def equals_naive(pu, nv):
    keys = nv.keys_in_order()
    assert pu.n_bins() == len(keys)
    got = table(pu)
    bad = [(i, k) for i, k in enumerate(keys) if pn.words_of(got[i]) != nv.bins.get(k, [0, 0, 0, 0])]
    assert not bad, (bad[:4], [pn.words_of(got[i]) for i, _ in bad[:4]], [nv.bins.get(k) for _, k in bad[:4]])
    assert pu.counters() == nv.counters(), (pu.counters(), nv.counters())
    rid, pos, fwd = pu.locate(np.arange(len(keys), dtype=np.uint64))
    assert [(int(r), int(p), 0 if f else 1) for r, p, f in zip(rid, pos, fwd)] == keys
    return got


def both(pu, nv, rid, pos, fwd, level, smp_n, shared=None):
    pu.add(rid, pos, fwd, level, smp_n, shared)
    nv.add(rid, pos, fwd, level, smp_n, shared)


# ------------------------------------------------------------------ array mode
def case_one_bin(X):
    """1. 3 * 1024 + 100 records, four workgroups of k_pileup_accum, all at one (p, strand): the five words equal the naive sums"""
    rng = np.random.default_rng(1)
    n = 3 * RECS_PER_BLOCK + 100
    regions = [(0, 500, 600)]
    for fwd in (1, 0):
        pu, nv = X.pileup(regions), pn.Naive(regions)
        both(pu, nv, np.zeros(n, np.int32), np.full(n, 537), np.full(n, fwd), rng.uniform(-100, 150, n).astype(np.float32), rng.integers(1, 40, n))
        got = equals_naive(pu, nv)
        assert int(got["n"].sum()) == n and int(got["n"][2 * 37 + (0 if fwd else 1)]) == n and pu.counters() == (0, 0, n)


def case_carry(X):
    """2. 16 records of +-2047.99 in one bin: SS_hi is not zero, S is negative; a second call carries in global memory again"""
    regions = [(0, 500, 600)]
    pu, nv = X.pileup(regions), pn.Naive(regions)
    lv = np.array([2047.99] * 5 + [-2047.99] * 11, np.float32)
    args = (np.zeros(16, np.int32), np.full(16, 500), np.ones(16, np.uint32), lv, np.arange(16))
    both(pu, nv, *args)
    got = equals_naive(pu, nv)
    assert int(got["SS_hi"][0]) > 0 and int(got["S"][0]) < 0 and int(got["n"][0]) == 16 and int(got["D"][0]) == 120
    both(pu, nv, *args)
    got = equals_naive(pu, nv)
    assert int(got["SS_hi"][0]) == nv.bins[(0, 500, 0)][2] >> 64 >= 2


def case_dropped_skipped_outside(X):
    """3. NaN, +-inf and +-2048 are dropped; shared == 1 is skipped without KEEP_SHARED and added with it; p = en - 4 and p = st - 1
    are outside, p = st and p = en - 5 the region's first and last bin; a bad rid is refused and the table stays as it was"""
    regions = [(0, 700, 760)]
    lv = np.array([np.nan, np.inf, -np.inf, 2048.0, -2048.0, 2047.99, 80.0, 90.0, 70.0, 71.0, 72.0, 73.0], np.float32)
    pos = np.array([710, 711, 712, 713, 714, 715, 716, 716, 756, 699, 700, 755])
    sh = np.array([0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0], np.uint32)
    n = lv.size
    for keep in (False, True):
        pu, nv = X.pileup(regions, keep), pn.Naive(regions, keep)
        both(pu, nv, np.zeros(n, np.int32), pos, np.ones(n), lv, np.full(n, 9), sh)
        got = equals_naive(pu, nv)
        assert pu.counters() == (5, 2, 5 if keep else 4)
        assert int(got["n"][0]) == 1 and int(got["n"][-2]) == 1 and int(got["n"][2 * 16]) == (2 if keep else 1) and pu.n_bins() == 2 * 56
        before = table(pu).tobytes(), pu.counters()
        for bad in (-1, 1, 7):
            rid = np.array([0, bad, 0], np.int32)
            rc = X.L.unc_pileup_add(pu.h, 3, rid.ctypes.data, np.full(3, 720, np.uint64).ctypes.data, np.ones(3, np.uint32).ctypes.data,
                                    np.full(3, 80, np.float32).ctypes.data, np.ones(3, np.uint32).ctypes.data, None, None)
            assert rc == ERR_ARG and X.L.unc_last_error()
        assert (table(pu).tobytes(), pu.counters()) == before
        pu.reset()
        assert not table(pu).view(np.uint64).any() and pu.counters() == (0, 0, 0)


def case_strands(X):
    """4. the same p with fwd = 1 and fwd = 0 lands in two bins; locate returns what was put in"""
    regions = [(0, 100, 200)]
    pu, nv = X.pileup(regions), pn.Naive(regions)
    both(pu, nv, [0, 0, 0], [150, 150, 150], [1, 0, 0], np.array([80, 90, 91], np.float32), [5, 6, 7])
    got = equals_naive(pu, nv)
    hit = np.flatnonzero(got["n"])
    assert list(hit) == [100, 101] and list(got["n"][hit]) == [1, 2] and list(got["D"][hit]) == [5, 13]
    rid, pos, fwd = pu.locate(hit)
    assert list(rid) == [0, 0] and list(pos) == [150, 150] and list(fwd) == [1, 0]


def random_records(rng, n, lo, hi):
    return (np.zeros(n, np.int32), rng.integers(lo, hi, n), rng.integers(0, 2, n), (rng.standard_normal(n) * 300).astype(np.float32),
            rng.integers(1, 60, n), (rng.random(n) < 0.1).astype(np.uint32))


def case_order_and_split(X):
    """5. the same 5 000 random records in one call, then shuffled in 7 calls: gather over all bins gives identical bytes"""
    rng = np.random.default_rng(5)
    regions = [(0, 1000, 1404)]
    rec = random_records(rng, 5000, 990, 1410)
    one, seven, nv = X.pileup(regions), X.pileup(regions), pn.Naive(regions)
    both(one, nv, *rec)
    perm = rng.permutation(5000)
    for part in np.array_split(perm, 7):
        seven.add(*[a[part] for a in rec])
    assert table(one).tobytes() == table(seven).tobytes() and one.counters() == seven.counters()
    equals_naive(one, nv)
    assert nv.outside > 0 and nv.added > 4000
    return one


def stretch_records(rng, stretch, row_first=0):
    """what a round would add for a stretch: one record per row, at the row's position"""
    rid, st, en, fwd = stretch
    rows = np.arange(row_first, en - st - 4)
    pos = st + rows if fwd else en - 5 - rows
    n = rows.size
    return (np.full(n, rid, np.int32), pos, np.full(n, 1 if fwd else 0), rng.uniform(60, 120, n).astype(np.float32), rng.integers(1, 30, n),
            np.zeros(n, np.uint32))


def case_regions(X):
    """6. two regions with a gap and one of 4 bases (no bins), given unsorted; a forward and a minus stretch cross both regions and the
    gap: the bins in the regions are filled, the rows in the gap (and the k-mers that hang over a region's end) are outside.  Then
    the default, all sequences whole"""
    rng = np.random.default_rng(6)
    regions = [(0, 2100, 2160), (0, 2050, 2054), (0, 2000, 2040)]
    pu, nv = X.pileup(regions), pn.Naive(regions)
    assert pu.n_bins() == 2 * (36 + 0 + 56)
    for s in ((0, 1990, 2170, True), (0, 1985, 2175, False)):
        both(pu, nv, *stretch_records(rng, s))
    equals_naive(pu, nv)
    # 176 and 186 rows; 36 + 56 positions of each lie in a region
    assert nv.added == 2 * 92 and nv.outside == (176 - 92) + (186 - 92)
    pu, nv = X.pileup(), pn.Naive(whole(X))
    assert pu.n_bins() == 2 * (X.seq_len - 4)
    both(pu, nv, [0] * 5, [0, X.seq_len - 5, X.seq_len - 4, 4321, 4321], [1, 0, 1, 1, 0], np.array([80, 81, 82, 83, 84], np.float32), [3] * 5)
    assert pu.counters() == (0, 1, 4)
    bins = pu.covered(1)
    assert list(bins) == [0, 2 * 4321, 2 * 4321 + 1, 2 * (X.seq_len - 5) + 1] == nv.covered(1)
    assert [pn.words_of(w) for w in pu.gather(bins)] == [nv.bins[k] for k in ((0, 0, 0), (0, 4321, 0), (0, 4321, 1), (0, X.seq_len - 5, 1))]


# ------------------------------------------------------------------ through the alignment
def batch(R):
    """model_cases' batch on stretches of the example reference: six queries of 50 rows whose stretches overlap, strands alternating,
    and a seventh of 60 rows on another read"""
    qs = [(0, 300 * i, 300 * i + 1000) for i in range(6)] + [(2, 0, 0)]
    stretches = [(0, 100 + 37 * i, 154 + 37 * i, i % 2 == 0) for i in range(6)] + [(0, 5000, 5064, False)]
    return qs, stretches


def row_pos(stretch, row):
    _, st, en, fwd = stretch
    return st + row if fwd else en - 5 - row


def naive_of_segments(regions, stretches, segs, info, keep_shared=False):
    nv = pn.Naive(regions, keep_shared)
    for s, seg, inf in zip(stretches, segs, info):
        assert seg.size == int(inf["n_rows"])
        rows = int(inf["row_first"]) + np.arange(seg.size)
        nv.add([s[0]] * seg.size, [row_pos(s, int(r)) for r in rows], [1 if s[3] else 0] * seg.size, seg["level"], seg["smp_n"], seg["shared"])
    return nv


def same_outputs(a, b):
    assert a[0].tobytes() == b[0].tobytes()
    for i in (1, 2, 3):
        for x, y in zip(a[i], b[i]):
            assert (x is None and y is None) or x.tobytes() == y.tobytes()
    assert all(sc.rec_equal(x, y) for x, y in zip(a[4], b[4])) and a[5].tobytes() == b[5].tobytes()


def raw_call(X, R, qs, stretches, pileup, seg_room=None, kmers=False, acc=None):
    """unc_align_pileup_call through the record itself: seg_room None = no segs at all, a number = that many records of room a query;
    kmers: the rows as k-mer arrays instead of coordinates -> (rc, info, seg)"""
    from uncalled_amd import capi
    n = len(qs)
    q = np.zeros(n, capi.ALIGN_QUERY)
    for i, (r, st, en) in enumerate(qs):
        q[i]["read"], q[i]["smp_st"], q[i]["smp_en"] = r, st, en
    res = np.zeros(n, capi.ALIGN_RESULT)
    ss = capi._stretches(stretches)
    rec = capi.AlignCall()
    rec.size = C.sizeof(capi.AlignCall)
    rec.n_reads, rec.raw, rec.offsets, rec.calib = len(R.signals), R.raw.ctypes.data, R.offsets.ctypes.data, R.calib.ctypes.data
    rec.n_queries, rec.queries, rec.results = n, q.ctypes.data, res.ctypes.data
    keep = []
    if kmers:
        kms = [capi.ref_kmers(X.index, X.prefix, *s) for s in stretches]
        km = np.concatenate(kms + [np.zeros(1, np.uint16)])
        km_off = np.cumsum([0] + [k.size for k in kms]).astype(np.uint64)
        rec.kmers, rec.km_off = km.ctypes.data, km_off.ctypes.data
        keep += [km, km_off]
    else:
        rec.refseq, rec.stretches = X.refseq.h, ss.ctypes.data
    info = seg = None
    if seg_room is not None:
        seg = np.zeros(max(1, seg_room * n), capi.SEGMENT)
        seg_off = (seg_room * np.arange(n + 1)).astype(np.uint64)
        info = np.zeros(n, capi.SEG_INFO)
        so = capi.AlignSegments()
        so.seg, so.seg_off, so.info = seg.ctypes.data, seg_off.ctypes.data, info.ctypes.data
        rec.segs = C.cast(C.pointer(so), C.c_void_p)
        keep += [so, seg_off]
    if acc is not None:
        rec.accumulate = acc.h
    rc = X.L.unc_align_pileup_call(C.byref(rec), pileup.h if pileup is not None else None)
    return rc, res, info, seg


def case_through_the_alignment(X, R):
    """7. unc_align_pileup_call on the segment cases' reads, both strands, with a band and without, with rows that may be cut, and
    with a workspace that forces three rounds or more: the pile-up equals the naive pile-up of the call's own segments, info and
    stretches; kmers_out[row] is stats' k-mer of the bin the row went to; results, levels, path, segments and statuses are those of
    the call without a pile-up.  The same table with seg == NULL and with a seg room of three records a query: as with an
    accumulator (case_align_short_room), the records on the device do not depend on the caller's room"""
    from uncalled_amd import capi
    qs, stretches = batch(R)
    regions = whole(X)
    first = None
    for o, ws in ((None, 0), (capi.align_opts(band=40), 0), (sc._ev(subseq=1), 0), (None, 6200)):
        for keep in (False, True):
            pu = X.pileup(None, keep)
            out = capi.align_ref_batch(X.refseq, R.raw, R.offsets, R.calib, qs, stretches, o, workspace_bytes=ws, levels=True, paths=True,
                                       kmers=True, segments=True, pileup=pu)
            res, _, _, kms, segs, info = out
            assert (res["status"] == capi.DTW_OK).all() and (info["status"] == capi.SEG_OK).all()
            if ws:
                assert capi.dtw_last_timing(X.L)[1] >= 3
            nv = naive_of_segments(regions, stretches, segs, info, keep)
            assert nv.added > 100 and nv.outside == 0 and nv.dropped == 0
            if o is None:       # 360 rows, some of them on an event they share with the row before
                assert nv.added > 300 and (keep or nv.added < sum(int(x) for x in info["n_rows"]))
            equals_naive(pu, nv)
            same_outputs(out, capi.align_ref_batch(X.refseq, R.raw, R.offsets, R.calib, qs, stretches, o, workspace_bytes=ws, levels=True,
                                                   paths=True, kmers=True, segments=True))
            # the strand rule: the k-mer the DTW saw in a row is the k-mer of the bin the row's record went to
            for s, km, inf in zip(stretches, kms, info):
                rows = int(inf["row_first"]) + np.arange(int(inf["n_rows"]))
                bins = np.array([2 * row_pos(s, int(r)) + (0 if s[3] else 1) for r in rows], np.uint64)
                assert np.array_equal(pu.stats(bins)["kmer"], km[rows]), s
            if o is None and not keep:
                if ws == 0:
                    first = table(pu).tobytes(), pu.counters()
                assert (table(pu).tobytes(), pu.counters()) == first       # the rounds do not change the table
    # rows cut: some alignment must start behind row 0 for the case to say something about row_first
    pu = X.pileup()
    _, segs, info = capi.align_ref_batch(X.refseq, R.raw, R.offsets, R.calib, qs[:1], [(0, 100, 400, False)], sc._ev(subseq=1), segments=True,
                                         pileup=pu)
    assert int(info["row_first"][0]) > 0 or int(info["n_rows"][0]) < 296
    equals_naive(pu, naive_of_segments(regions, [(0, 100, 400, False)], segs, info))
    # the caller's room
    for room in (None, 3):
        pu = X.pileup()
        rc, res, info, seg = raw_call(X, R, qs, stretches, pu, room)
        assert rc == 0, X.L.unc_last_error()
        assert (res["status"] == capi.DTW_OK).all() and (room is None or (info["status"] == capi.SEG_TRUNCATED).all())
        assert (table(pu).tobytes(), pu.counters()) == first
    # regions with gaps under the stretches: rows in the gaps are outside
    regions = [(0, 120, 200), (0, 230, 300), (0, 5010, 5014)]
    pu = X.pileup(regions)
    _, segs, info = capi.align_ref_batch(X.refseq, R.raw, R.offsets, R.calib, qs, stretches, segments=True, pileup=pu)
    nv = naive_of_segments(regions, stretches, segs, info)
    assert nv.outside > 60 and nv.added > 100
    equals_naive(pu, nv)
    # a query without a path contributes nothing
    pu = X.pileup()
    res, segs, info = capi.align_ref_batch(X.refseq, R.raw, R.offsets, R.calib, qs[:2] + [(0, 0, 300)], stretches[:2] + [(0, 900, 944, True)],
                                           capi.align_opts(max_events=80), segments=True, pileup=pu)
    assert list(res["status"]) == [capi.ALIGN_TOO_MANY, capi.ALIGN_TOO_MANY, capi.DTW_OK] and int(info["status"][0]) == capi.SEG_NONE
    equals_naive(pu, naive_of_segments(whole(X), stretches[:2] + [(0, 900, 944, True)], segs, info))


def case_with_an_accumulator(X, R):
    """8. an accumulator and a pile-up in one call: the accumulator's sums are those of the call without the pile-up, the pile-up
    those of the call without the accumulator"""
    from uncalled_amd import capi
    qs, stretches = batch(R)
    alone, pu_alone = capi.ModelAcc(lib=X.L), X.pileup()
    capi.align_ref_batch(X.refseq, R.raw, R.offsets, R.calib, qs, stretches, accumulate=alone)
    capi.align_ref_batch(X.refseq, R.raw, R.offsets, R.calib, qs, stretches, pileup=pu_alone)
    for ws in (0, 6200):
        acc, pu = capi.ModelAcc(lib=X.L), X.pileup()
        res = capi.align_ref_batch(X.refseq, R.raw, R.offsets, R.calib, qs, stretches, workspace_bytes=ws, accumulate=acc, pileup=pu)
        assert (res["status"] == capi.DTW_OK).all()
        assert all(np.array_equal(a, b) for a, b in zip(acc.read()[:4], alone.read()[:4])) and acc.read()[4] == alone.read()[4]
        assert int(acc.read()[0].sum()) > 300
        assert table(pu).tobytes() == table(pu_alone).tobytes() and pu.counters() == pu_alone.counters()
    return pu


# ------------------------------------------------------------------ covered, statistics, merge
def fill(pu, nv, bins, rng, most=3):
    """1..most records in each listed bin of a one-region pile-up that starts at position 10"""
    bins = np.repeat(np.asarray(bins, np.int64), rng.integers(1, most + 1, len(bins)))
    n = bins.size
    if n:
        both(pu, nv, np.zeros(n, np.int32), 10 + bins // 2, 1 - bins % 2, rng.uniform(60, 120, n).astype(np.float32), np.full(n, 4))


def case_covered(X):
    """9. tables of 2, 62, 64, 66, 1022, 1024, 1026 and 3074 bins (a wavefront's step, a workgroup's chunk and three chunks, each
    with the even counts around it); none, all and a random third covered; min_cov 1, 2 and above the largest count; pair mode; a
    cap below the count.  The list is ascending and equals the naive list"""
    rng = np.random.default_rng(9)
    for nb in (2, 62, 64, 66, SCAN_CHUNK - 2, SCAN_CHUNK, SCAN_CHUNK + 2, 3 * SCAN_CHUNK + 2):
        regions = [(0, 10, 10 + nb // 2 + 4)]
        none, every, third = (X.pileup(regions) for _ in range(3))
        n_none, n_every, n_third = (pn.Naive(regions) for _ in range(3))
        assert none.n_bins() == nb
        fill(every, n_every, np.arange(nb), rng)
        fill(third, n_third, np.flatnonzero(rng.random(nb) < 1 / 3), rng)
        for min_cov in (1, 2, 4):
            assert list(none.covered(min_cov)) == []
            for pu, nv in ((every, n_every), (third, n_third)):
                got = pu.covered(min_cov)
                assert list(got) == nv.covered(min_cov), (nb, min_cov)
                assert (np.diff(got.astype(np.int64)) > 0).all()
            assert list(third.covered(min_cov, other=every)) == n_third.covered(min_cov, n_every), (nb, min_cov)
            assert list(every.covered(min_cov, other=none)) == []
        assert list(every.covered(1)) == list(range(nb))
        want = n_every.covered(2)
        got, full = every.covered(2, cap=len(want) // 2)
        assert full == len(want) and list(got) == want[:len(want) // 2]
        got, full = every.covered(1, other=third, cap=1)
        assert full == len(n_third.covered(1)) and list(got) == n_third.covered(1)[:1]
    return every


def case_stats_and_compare(X):
    """10. the doubles of stats and compare equal pileup_naive's bit for bit (compared as uint64): a bin with V == 0, one with
    n == 1, an empty one, both strands, the r9.4 template and a custom model; se2 == 0 gives t = 0"""
    from uncalled_amd import capi
    rng = np.random.default_rng(10)
    regions = [(0, 200, 300)]
    a, b = X.pileup(regions), X.pileup(regions)
    na, nb_ = pn.Naive(regions), pn.Naive(regions)
    # positions: 210 many random records on both strands, 220 three identical levels (V == 0), 230 one record, 240 nothing
    def recs(n, pos, fwd, lv):
        return np.zeros(n, np.int32), np.full(n, pos), np.full(n, fwd), np.asarray(lv, np.float32), rng.integers(1, 50, n), None
    for pu, nv, shift in ((a, na, 0.0), (b, nb_, 1.5)):
        both(pu, nv, *recs(40, 210, 1, rng.normal(85 + shift, 2, 40)))
        both(pu, nv, *recs(33, 210, 0, rng.normal(95 + shift, 3, 33)))
        both(pu, nv, *recs(3, 220, 1, [81.25] * 3))
        both(pu, nv, *recs(2, 250, 0, rng.normal(-3 + shift, 1, 2)))
    both(a, na, *recs(1, 230, 1, [77.0]))
    keys = na.keys_in_order()
    bins = np.array([keys.index(k) for k in ((0, 210, 0), (0, 210, 1), (0, 220, 0), (0, 230, 0), (0, 240, 0), (0, 250, 1))], np.uint64)
    custom = capi.Model.from_pairs(mc.random_pairs(15), lib=X.L)
    for model, pairs in ((None, capi.Model.default(lib=X.L).pairs()), (custom, custom.pairs())):
        got = a.stats(bins, model)
        for i, bin_ in enumerate(bins):
            rid, pos, strand = keys[int(bin_)]
            km = int(capi.ref_kmers(X.index, X.prefix, rid, pos, pos + 5, strand == 0)[0])
            assert int(got["kmer"][i]) == km
            assert got["model_mean"][i].tobytes() == pairs[km, 0].tobytes() and got["model_stdv"][i].tobytes() == pairs[km, 1].tobytes()
            n, mean, sd, dwell, z = pn.stats(na.bins.get(keys[int(bin_)]), pairs[km, 0], pairs[km, 1])
            assert int(got["n"][i]) == n
            assert [int(x) for x in pn.bits([got["mean"][i], got["sd"][i], got["dwell"][i], got["z"][i]])] == \
                [int(x) for x in pn.bits([mean, sd, dwell, z])], (i, got[i], (mean, sd, dwell, z))
    got = a.stats(bins)
    assert list(got["n"]) == [40, 33, 3, 1, 0, 2] and got["sd"][2] == 0 and got["sd"][3] == 0 and got["mean"][2] == 81.25
    assert not got[4]["mean"] and not got[4]["z"] and abs(got["mean"][0] - 85) < 2 and abs(got["sd"][0] - 2) < 1
    both_have = bins[[0, 1, 2, 5]]
    cmp_ = a.compare(b, both_have)
    for i, bin_ in enumerate(both_have):
        k = keys[int(bin_)]
        ma, mb, se2, t = pn.compare(na.bins[k], nb_.bins[k])
        assert [int(x) for x in pn.bits([cmp_["mean_a"][i], cmp_["mean_b"][i], cmp_["se2"][i], cmp_["t"][i]])] == \
            [int(x) for x in pn.bits([ma, mb, se2, t])], (i, cmp_[i])
        assert (int(cmp_["n_a"][i]), int(cmp_["n_b"][i])) == (na.bins[k][0], nb_.bins[k][0])
    assert cmp_["se2"][2] == 0 and cmp_["t"][2] == 0 and cmp_["t"][0] < -1
    same = a.compare(a, both_have)
    assert not same["t"].any()
    for lone in (bins[3:4], bins[4:5]):       # n == 1 in a, nothing in b; nothing in either
        out = np.zeros(1, capi.PILEUP_CMP)
        assert X.L.unc_pileup_compare(a.h, b.h, 1, lone.ctypes.data, out.ctypes.data) == ERR_ARG and not out.view(np.uint8).any()


def case_merge(X):
    """11. A.merge(B) equals one object fed both record sets, counters included; other regions are refused"""
    rng = np.random.default_rng(11)
    regions = [(0, 3000, 3200), (0, 3300, 3310)]
    one, two = random_records(rng, 3000, 2990, 3320), random_records(rng, 2000, 2990, 3320)
    # a bin whose low words wrap when added
    big = (np.zeros(3, np.int32), np.full(3, 3100), np.ones(3), np.full(3, 2047.99, np.float32), np.full(3, 1), np.zeros(3, np.uint32))
    A, B, Cc = X.pileup(regions), X.pileup(regions), X.pileup(regions)
    nv = pn.Naive(regions)
    A.add(*one); A.add(*big)
    B.add(*two); B.add(*big)
    for r in (one, big, two, big):
        both(Cc, nv, *r)
    A.merge(B)
    assert table(A).tobytes() == table(Cc).tobytes() and A.counters() == Cc.counters()
    got = equals_naive(A, nv)
    assert int(got["SS_hi"][2 * 100]) >= 1
    other = X.pileup([(0, 3000, 3200), (0, 3300, 3311)])
    for x, y in ((A, other), (other, A), (A, A)):
        assert X.L.unc_pileup_merge(x.h, y.h) == ERR_ARG
    assert table(A).tobytes() == table(Cc).tobytes()


def case_refusals(X, R):
    """12. before the device: pileup= with k-mer arrays; a pile-up of another RefSeq; overlapping regions (and the other bad regions);
    covered with min_cov == 0 or a pile-up of other regions; gather of a bin that does not exist"""
    from uncalled_amd import capi
    qs, stretches = batch(R)
    pu = X.pileup()
    rc, res, _, _ = raw_call(X, R, qs, stretches, pu, kmers=True)
    assert rc == ERR_ARG and b"coordinates" in X.L.unc_last_error() and not res.view(np.uint8).any()
    rc, res, _, _ = raw_call(X, R, qs, stretches, None, kmers=True)      # without a pile-up the same record is unc_align_call's
    assert rc == 0 and (res["status"] == capi.DTW_OK).all()
    with pytest.raises(ValueError):
        capi.align_batch(R.raw, R.offsets, R.calib, qs[:1], [R.walk[:50]], lib=X.L, pileup=pu)
    other = capi.RefSeq(X.index, X.prefix)
    foreign = capi.Pileup(other, lib=X.L)
    rc, res, _, _ = raw_call(X, R, qs, stretches, foreign)
    assert rc == ERR_ARG and not res.view(np.uint8).any()
    assert pu.counters() == (0, 0, 0) and foreign.counters() == (0, 0, 0)
    for bad in ([(0, 100, 200), (0, 199, 300)], [(0, 100, 200), (0, 150, 160)], [(0, 100, 200), (0, 100, 200)], [(1, 0, 10)], [(-1, 0, 10)],
                [(0, 20, 10)], [(0, 0, X.seq_len + 1)]):
        rg = capi._stretches([(r, s, e, True) for r, s, e in bad])
        h = C.c_void_p()
        assert X.L.unc_pileup_create(X.refseq.h, len(bad), rg.ctypes.data, 0, C.byref(h)) == ERR_ARG and not h.value, bad
    X.pileup([(0, 100, 200), (0, 200, 300), (0, 300, 300), (0, 300, 303)])       # touching regions and empty ones are legal
    n = C.c_uint64()
    assert X.L.unc_pileup_covered(pu.h, None, 0, None, 0, C.byref(n)) == ERR_ARG
    assert X.L.unc_pileup_covered(pu.h, X.pileup([(0, 0, 100)]).h, 1, None, 0, C.byref(n)) == ERR_ARG
    out = np.zeros(5, np.uint64)
    assert X.L.unc_pileup_gather(pu.h, 1, np.array([pu.n_bins()], np.uint64).ctypes.data, out.ctypes.data) == ERR_ARG and not out.any()
    foreign.close()
    other.close()


def case_layout(L):
    """13. the call's record is still 200 bytes; the new entry points are declared in the header and exported"""
    import re
    from pathlib import Path
    from uncalled_amd import capi
    assert C.sizeof(capi.AlignCall) == 200 and capi.AlignCall.accumulate.offset == 184
    assert capi.PILEUP_STAT.itemsize == 56 and capi.PILEUP_CMP.itemsize == 64 and capi.PILEUP_WORDS.itemsize == 40
    txt = (Path(__file__).resolve().parents[1] / "include" / "uncalled_hip.h").read_text()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in ("create", "free", "reset", "device_bytes", "n_bins", "counters", "add", "last_timing", "covered", "gather", "bin_locate",
                 "merge", "stats", "compare"):
        assert re.search(r"\bunc_pileup_%s\s*\(" % name, txt), name
        assert hasattr(L, "unc_pileup_" + name), name
    assert re.search(r"\bunc_align_pileup_call\s*\(", txt) and hasattr(L, "unc_align_pileup_call")
