"""The cases of the signal pile-up (k_pileup.hip, unc_pileup.cpp), shared by tests/test_pileup_cpu.py (the lanesim emulator) and
tests/test_gpu_pileup.py (the MI355X).  X is the context under test: the library (capi.load's handle), the bundled 10 kb example
index and its packed reference.  The independent checker is tests/pileup_naive.py (Python integers, dictionaries keyed
(rid, pos, strand)); the reads are those of tests/segments_cases.py.

The kernels' grid rules (pileup_dev.h), which the shapes below straddle: k_pileup_accum takes 1024 records a workgroup; the
covered-bin kernels take 1024 bins a workgroup, 64 a wavefront's step.  Bins come in strand pairs, so a table's bin count is even:
where a count of bins is named, the cases use the even counts on both sides of it (2, 62, 64, 66, 1022, 1024, 1026, 3074).
k_pileup_scan is one workgroup that takes the per-workgroup counts 256 a pass with a running total, so a table of more than
256 * 1024 = 262 144 bins needs a second pass: the bundled example (19 992 bins) never does, the five-sequence reference of cases 15
to 18 (refalign_cases.multi_reference: 528 106 bins, 516 counts) takes three, the last of 4 counts.  In alignment mode
k_pileup_accum's grid is ceil(rows of the round / 1024), at most one workgroup an alignment, and workgroup b takes the alignments
b, b + grid, ...: a round of the example's batches (360 rows at most) is one workgroup, case 18's round of 2 209 rows is three
workgroups over eight alignments."""
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
    def __init__(self, L, prefix, seqs=None):
        """seqs: the sequences as strings, where the reference was made by the tests"""
        from uncalled_amd import capi
        self.L, self.prefix, self.seqs = L, prefix, seqs
        self.index = capi.Index(prefix, lib=L)
        self.refseq = capi.RefSeq(self.index, prefix)
        self.seq_len = int(self.index.seq_len(0))
        self.lens = [int(self.index.seq_len(r)) for r in range(len(self.index.seq_names()))]

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


# ------------------------------------------------------------------ five sequences, a table of three scan passes
# M is the context of refalign_cases.multi_reference: sequences of 141, 4, 131075, 150 and 132703 bases.  Its default table has
# 528 106 bins, 516 workgroups of the covered-bin kernels, three passes of k_pileup_scan; sequence 1 holds no bin.
SCAN_PASS = 256 * SCAN_CHUNK


def every(M):
    return [(r, 0, n) for r, n in enumerate(M.lens)]


def equals_naive_big(pu, nv):
    """equals_naive for a table of 10^5 bins and more: every bin's words are compared as there, the empty ones as arrays"""
    got = table(pu)
    assert got.size == pu.n_bins() == 2 * sum(max(0, en - st - 4) for _, st, en in nv.regions)
    held = np.flatnonzero(got.view(np.uint64).reshape(-1, 5).any(axis=1))
    want = sorted((nv.bin_of(k), k, b) for k, b in nv.bins.items())
    stray, missing = sorted(set(held.tolist()) - {i for i, _, _ in want}), sorted({i for i, _, _ in want} - set(held.tolist()))
    assert not stray and not missing, "%d bins hold something where the naive table is empty, from %s; %d are empty that should hold something, from %s" % (
        len(stray), [nv.key_of(i) for i in stray[:3]], len(missing), [nv.key_of(i) for i in missing[:3]])
    bad = [(i, k) for i, k, b in want if pn.words_of(got[i]) != b]
    assert not bad, (bad[:4], [pn.words_of(got[i]) for i, _ in bad[:4]], [nv.bins[k] for _, k in bad[:4]])
    assert pu.counters() == nv.counters(), (pu.counters(), nv.counters())
    rid, pos, fwd = pu.locate(held)
    where = [(int(r), int(p), 0 if f else 1) for r, p, f in zip(rid, pos, fwd)]
    bad = [(i, w, k) for w, (i, k, _) in zip(where, want) if w != k]
    assert not bad, "locate: %d of %d bins, the first (bin, got, naive) %s" % (len(bad), len(want), bad[:3])
    return got


def records_at(rng, keys, shift=0.0):
    """one record per (rid, pos, strand) key"""
    n = len(keys)
    return (np.array([k[0] for k in keys], np.int32), np.array([k[1] for k in keys], np.uint64), np.array([1 - k[2] for k in keys], np.uint32),
            rng.uniform(60 + shift, 120 + shift, n).astype(np.float32), rng.integers(1, 30, n), np.zeros(n, np.uint32))


def case_sequences(M):
    """15. array mode over five sequences.  The k-mers that would hang over a sequence's end and every position of the sequence
    without a bin are outside and leave the table empty, the next sequence's first bins included; the first and the last bin of every
    sequence on both strands; 4 000 random records over all sequences, their rids in no order.  Then regions of sequences 4, 0 and 2
    given unsorted, one of 4 bases between them, two that end at their sequence's last base, under stretches that cross them; what
    unc_pileup_add and unc_pileup_create refuse on five sequences"""
    from uncalled_amd import capi
    rng = np.random.default_rng(15)
    lens = M.lens
    assert lens == [141, 4, 131075, 150, 132703]
    regions = every(M)
    pu, nv = M.pileup(), pn.Naive(regions)
    assert pu.n_bins() == 528106
    over = [(r, p, s) for r in (0, 2, 3) for p in range(lens[r] - 4, lens[r]) for s in (0, 1)] + [(1, 0, 0), (1, 3, 1)]
    both(pu, nv, *records_at(rng, over))
    assert nv.counters() == (0, 26, 0) and pu.counters() == (0, 26, 0)
    got = table(pu)
    assert not got.view(np.uint64).any()
    for r in (2, 3, 4):       # (said again for the bins an offset without its sequence would have hit)
        assert not got[nv.bin_of((r, 0, 0)):nv.bin_of((r, 0, 0)) + 8].view(np.uint64).any()
    edges = [(r, p, s) for r in (0, 2, 3, 4) for p in (0, lens[r] - 5) for s in (0, 1)]
    both(pu, nv, *records_at(rng, edges))
    n = 4000
    rid = rng.integers(0, 5, n)
    pos = np.array([rng.integers(0, lens[r] + 2) for r in rid])
    lv = (rng.standard_normal(n) * 300).astype(np.float32)
    lv[::500] = np.inf
    both(pu, nv, rid, pos, rng.integers(0, 2, n), lv, rng.integers(1, 60, n), (rng.random(n) < 0.1).astype(np.uint32))
    assert (np.diff(rid) < 0).sum() > 1000
    got = equals_naive(pu, nv)
    assert nv.counters() == (5, 805, 2852), nv.counters()       # the naive checker's: 26 + 779 outside, 16 + 2836 added
    first = [nv.bin_of((r, 0, 0)) for r in (0, 2, 3, 4)]
    assert first == [0, 274, 274 + 262142, 274 + 262142 + 292] and all(int(got["n"][b]) >= 1 and int(got["n"][b + 1]) >= 1 for b in first)
    assert all(int(got["n"][b - 1]) >= 1 and int(got["n"][b - 2]) >= 1 for b in first[1:] + [528106])

    regions = [(4, 132603, 132703), (0, 20, 100), (2, 131000, 131075), (4, 10, 14), (2, 600, 700), (2, 500, 560)]
    pu, nv = M.pileup(regions), pn.Naive(regions)
    assert pu.n_bins() == 2 * (96 + 76 + 71 + 0 + 96 + 56)
    for s in ((2, 480, 720, True), (2, 470, 730, False), (2, 130950, 131075, False), (2, 130940, 131075, True), (4, 132500, 132703, True),
              (4, 132400, 132703, False), (0, 0, 141, True), (0, 0, 141, False), (4, 0, 50, False), (3, 0, 150, True),
              # in front of their sequence's first region, at positions that lie in the region of sequence 0
              (2, 0, 120, True), (2, 0, 130, False)):
        both(pu, nv, *stretch_records(rng, s))
    equals_naive(pu, nv)
    # the rows of the twelve stretches, and of each the positions that lie in a region
    assert nv.added == 2 * (56 + 96) + 2 * 71 + 2 * 96 + 2 * 76
    assert nv.outside == 236 + 256 + 121 + 131 + 199 + 299 + 2 * 137 + 46 + 146 + 116 + 126 - nv.added
    before = table(pu).tobytes(), pu.counters()
    for bad in (5, -1):
        rid = np.array([2, bad, 4], np.int32)
        rc = M.L.unc_pileup_add(pu.h, 3, rid.ctypes.data, np.full(3, 650, np.uint64).ctypes.data, np.ones(3, np.uint32).ctypes.data,
                                np.full(3, 80, np.float32).ctypes.data, np.ones(3, np.uint32).ctypes.data, None, None)
        assert rc == ERR_ARG and M.L.unc_last_error()
    for bad in ([(2, 0, 100), (5, 0, 100)], [(-1, 0, 100)], [(0, 0, 100), (3, 0, 151)], [(1, 0, 5)]):
        rg = capi._stretches([(r, s, e, True) for r, s, e in bad])
        h = C.c_void_p()
        assert M.L.unc_pileup_create(M.refseq.h, len(bad), rg.ctypes.data, 0, C.byref(h)) == ERR_ARG and not h.value, bad
    assert (table(pu).tobytes(), pu.counters()) == before
    M.pileup([(3, 0, 150), (1, 0, 4), (1, 4, 4)])


def boundary_bins(M, nv):
    """each sequence's first and last bin pair: the bins on both sides of every sequence boundary in bin order are among them"""
    return [nv.bin_of((r, p, s)) for r in (0, 2, 3, 4) for p in (0, M.lens[r] - 5) for s in (0, 1)]


def case_stats_sequences(M):
    """16. stats' k-mer is the k-mer of the FASTA string at the bin's (rid, pos, strand) and ref_kmers' of the same place, at each
    sequence's first and last bin pair (so on both sides of every boundary in bin order) and at 200 random bins; the model's pair is
    that k-mer's, the doubles equal pileup_naive's bit for bit, and so do compare's on bins of sequences 2 and 4"""
    from uncalled_amd import capi
    rng = np.random.default_rng(16)
    regions = every(M)
    a, b = M.pileup(), M.pileup()
    na, nb_ = pn.Naive(regions), pn.Naive(regions)
    edge = boundary_bins(M, na)
    assert sorted(edge) == sorted([0, 1, 528104, 528105] + [at + d for at in (274, 274 + 262142, 274 + 262142 + 292) for d in (-2, -1, 0, 1)])
    bins = np.array(edge + [int(x) for x in rng.integers(0, 528106, 200)], np.uint64)
    keys = [na.key_of(int(x)) for x in bins]
    assert {k[0] for k in keys} == {0, 2, 3, 4} and {k[2] for k in keys} == {0, 1}
    # records: three of four listed bins hold 1..4 in a; the listed bins of sequences 2 and 4 hold 2..5 in both
    some = [k for i, k in enumerate(keys) if i % 4]
    for k in some:
        both(a, na, *records_at(rng, [k] * int(rng.integers(1, 5))))
    pair = sorted({k for k in keys if k[0] in (2, 4)})[::3]
    assert len(pair) > 30 and {k[0] for k in pair} == {2, 4}
    for pu, nv, shift in ((a, na, 0.0), (b, nb_, 1.5)):
        for k in pair:
            both(pu, nv, *records_at(rng, [k] * int(rng.integers(2, 6)), shift))
    custom = capi.Model.from_pairs(mc.random_pairs(16), lib=M.L)
    for model, pairs in ((None, capi.Model.default(lib=M.L).pairs()), (custom, custom.pairs())):
        got = a.stats(bins, model)
        for i, (rid, pos, strand) in enumerate(keys):
            km = pn.py_kmer(M.seqs[rid], pos, strand == 0)
            assert int(got["kmer"][i]) == km, (i, rid, pos, strand)
            assert km == int(capi.ref_kmers(M.index, M.prefix, rid, pos, pos + 5, strand == 0)[0])
            assert got["model_mean"][i].tobytes() == pairs[km, 0].tobytes() and got["model_stdv"][i].tobytes() == pairs[km, 1].tobytes()
            n, mean, sd, dwell, z = pn.stats(na.bins.get((rid, pos, strand)), pairs[km, 0], pairs[km, 1])
            assert int(got["n"][i]) == n
            assert [int(x) for x in pn.bits([got["mean"][i], got["sd"][i], got["dwell"][i], got["z"][i]])] == \
                [int(x) for x in pn.bits([mean, sd, dwell, z])], (i, got[i], (mean, sd, dwell, z))
    assert sum(1 for k in keys if k in na.bins) > 150 and sum(1 for k in keys if k not in na.bins) > 20
    both_have = np.array([na.bin_of(k) for k in pair], np.uint64)
    cmp_ = a.compare(b, both_have)
    for i, k in enumerate(pair):
        ma, mb, se2, t = pn.compare(na.bins[k], nb_.bins[k])
        assert [int(x) for x in pn.bits([cmp_["mean_a"][i], cmp_["mean_b"][i], cmp_["se2"][i], cmp_["t"][i]])] == \
            [int(x) for x in pn.bits([ma, mb, se2, t])], (i, cmp_[i])
        assert (int(cmp_["n_a"][i]), int(cmp_["n_b"][i])) == (na.bins[k][0], nb_.bins[k][0])
    assert cmp_["t"].any()


def fill_bins(pu, nv, bins, rng, twice=()):
    """1..3 records in each listed bin of the table, two in each bin of `twice`"""
    bins = np.concatenate([np.repeat(np.asarray(bins, np.int64), rng.integers(1, 4, len(bins))), np.repeat(np.asarray(twice, np.int64), 2)])
    if bins.size:
        both(pu, nv, *records_at(rng, [nv.key_of(int(x)) for x in bins]))


def scan_edges(n_bins):
    """the first and the last bin of the workgroups on both sides of the scan's pass boundaries, of the first and of the last (a
    partial one)"""
    out = []
    for g in (0, 255, 256, 257, 511, 512, 515):
        out += [g * SCAN_CHUNK, min((g + 1) * SCAN_CHUNK, n_bins) - 1]
    return out


def scan_fills(rng, n_bins):
    edges = scan_edges(n_bins)
    assert edges[-1] == n_bins - 1 == 528105 and edges[-2] == 515 * SCAN_CHUNK
    thin = [int(x) for x in np.flatnonzero(rng.random(n_bins) < 1 / 200) if int(x) not in edges]
    return (("a", thin, edges),
            ("b", [x for x in thin if x >= SCAN_PASS], [x for x in edges if x >= SCAN_PASS]),
            ("c", [x for x in thin if x < SCAN_PASS], [x for x in edges if x < SCAN_PASS]),
            ("d", [], [n_bins - 1]),
            ("e", list(range(255 * SCAN_CHUNK, 257 * SCAN_CHUNK)), []))


def case_scan_passes(M, name, on_gpu=False):
    """17. k_pileup_scan past its first pass: 516 counts are three passes, the last of 4 counts.  One fill a call: on both sides of
    the pass boundaries (a), with nothing in the first pass (b), with nothing behind it (c), the table's last bin alone (d), two full
    workgroups astride the first boundary (e).  covered for min_cov 1 and 2, pair mode and the caps around the first pass' count equal
    the naive list and ascend"""
    rng = np.random.default_rng(17)
    regions = every(M)
    n_bins = 528106
    (thin, twice), = [f[1:] for f in scan_fills(rng, n_bins) if f[0] == name]
    pu, nv = M.pileup(), pn.Naive(regions)
    assert pu.n_bins() == n_bins
    fill_bins(pu, nv, thin, rng, twice)
    lists = {}
    for min_cov in (1, 2):
        got = pu.covered(min_cov)
        lists[min_cov] = want = nv.covered_of_bins(min_cov)
        first_bad = next((i for i, (x, y) in enumerate(zip(got.tolist(), want)) if x != y), min(got.size, len(want)))
        assert [int(x) for x in got] == want, "fill %s, min_cov %d: %d bins for %d, the first that differs at %d" % (name, min_cov, got.size, len(want), first_bad)
        assert (np.diff(got.astype(np.int64)) > 0).all() and len(want) > 0
        if on_gpu:
            assert all(t > 0 for t in pu.covered_last_timing())
    assert lists[1] == sorted(thin + twice) and set(twice) <= set(lists[2]) and len(lists[1]) * 50 < n_bins
    other, n_other = M.pileup(), pn.Naive(regions)
    fill_bins(other, n_other, [], rng, lists[1][::2])
    for min_cov in (1, 2):
        want = nv.covered_of_bins(min_cov, n_other)
        assert [int(x) for x in pu.covered(min_cov, other=other)] == want, min_cov
        assert min_cov == 2 or want == lists[1][::2]
    n1 = sum(1 for x in lists[1] if x < SCAN_PASS)
    n2 = sum(1 for x in lists[1] if SCAN_PASS <= x < 2 * SCAN_PASS)
    assert (n1 > 0) == (name in "ace") and (n2 > 0) == (name in "abe") and (len(lists[1]) > n1 + n2) == (name in "abd")
    # one below the number covered in the first pass, that number, one inside the second pass
    for cap in sorted({max(0, n1 - 1), n1, n1 + n2 // 2}):
        got, full = pu.covered(1, cap=cap)
        assert full == len(lists[1]) and [int(x) for x in got] == lists[1][:cap], cap


def case_scan_merge_gather(M):
    """17, continued, on the same table: A.merge(B) equals one object fed both fills, byte for byte over a gather of all covered bins,
    counters included; a gather of 100 000 listed bins drawn over the whole table, in no order and with repeats, equals the naive words"""
    from uncalled_amd import capi
    regions = every(M)
    n_bins = 528106
    A, B, Cc = M.pileup(), M.pileup(), M.pileup()
    nv = pn.Naive(regions)
    for pu, seed in ((A, 171), (B, 172)):
        _, thin, twice = scan_fills(np.random.default_rng(seed), n_bins)[0]
        fill_bins(pu, pn.Naive(regions), thin, np.random.default_rng(seed + 10), twice)       # the same records into both
        fill_bins(Cc, nv, thin, np.random.default_rng(seed + 10), twice)
    A.merge(B)
    cov = Cc.covered(1)
    want = nv.covered_of_bins(1)
    assert [int(x) for x in cov] == want == [int(x) for x in A.covered(1)], "covered: %d bins for %d" % (cov.size, len(want))
    assert A.gather(cov).tobytes() == Cc.gather(cov).tobytes() and A.counters() == Cc.counters() == nv.counters()
    assert int(A.gather(scan_edges(n_bins))["n"].min()) == 4
    equals_naive_big(A, nv)
    rng = np.random.default_rng(173)
    listed = np.concatenate([rng.integers(0, n_bins, 99000), rng.choice(cov, 999), [n_bins - 1]]).astype(np.uint64)
    rng.shuffle(listed)
    want = np.zeros(listed.size, capi.PILEUP_WORDS)
    held = {nv.bin_of(k): b for k, b in nv.bins.items()}
    hits = 0
    for i, x in enumerate(listed.tolist()):
        if x in held:
            n, S, SS, D = held[x]
            want[i] = (n, S, SS & (2 ** 64 - 1), SS >> 64, D)
            hits += 1
    assert hits > 1400 and listed.size == 100000
    assert Cc.gather(listed).tobytes() == want.tobytes()


def multi_batch(M):
    """eight queries of read 0 whole on eight stretches: 7 x 296 + 137 = 2 209 rows, a grid of three workgroups of k_pileup_accum for
    eight alignments.  Stretches 3, 5 and 7 (sequence 2, minus) and 4 and 6 (sequence 4, plus) overlap in pairs that fall to
    different workgroups of a stride of 3"""
    n2, n4 = M.lens[2], M.lens[4]
    qs = [(0, 0, 0)] * 8
    stretches = [(2, 0, 300, True), (4, n4 - 300, n4, False), (0, 0, 141, False), (2, n2 - 300, n2, False), (4, 100, 400, True),
                 (2, n2 - 450, n2 - 150, False), (4, 250, 550, True), (2, n2 - 600, n2 - 300, False)]
    assert sum(en - st - 4 for _, st, en, _ in stretches) == 2209
    return qs, stretches


MULTI_WS = 150000           # three rounds of multi_batch (two would hold 194 560 bytes of back-pointers, all eight 369 664)
MULTI_ROWS = [296, 296, 137, 296, 296, 296, 296, 296]


def aligned_pileup(M, R, o, ws):
    """one call of multi_batch with a pile-up over all sequences and every output: the pile-up equals the naive pile-up of the call's own
    segments, info and stretches; kmers_out[row] is stats' k-mer of the bin the row went to and the k-mer of the FASTA string there;
    the other outputs are those of the call without a pile-up -> (the table's bytes, the counters, info)"""
    from uncalled_amd import capi
    qs, stretches = multi_batch(M)
    kw = dict(workspace_bytes=ws, levels=True, paths=True, kmers=True, segments=True)
    pu = M.pileup()
    out = capi.align_ref_batch(M.refseq, R.raw, R.offsets, R.calib, qs, stretches, o, pileup=pu, **kw)
    rounds = capi.dtw_last_timing(M.L)[1]
    res, _, _, kms, segs, info = out
    assert (res["status"] == capi.DTW_OK).all() and (info["status"] == capi.SEG_OK).all()
    assert rounds >= 3 if ws else rounds == 1, rounds
    nv = naive_of_segments(every(M), stretches, segs, info)
    assert nv.outside == 0 and nv.dropped == 0 and nv.added > 1000
    got = equals_naive_big(pu, nv)
    same_outputs(out, capi.align_ref_batch(M.refseq, R.raw, R.offsets, R.calib, qs, stretches, o, **kw))
    for s, km, inf in zip(stretches, kms, info):
        rows = int(inf["row_first"]) + np.arange(int(inf["n_rows"]))
        bins = np.array([nv.bin_of((s[0], row_pos(s, int(r)), 0 if s[3] else 1)) for r in rows], np.uint64)
        assert np.array_equal(pu.stats(bins)["kmer"], km[rows]), s
        assert [int(x) for x in km[rows]] == [pn.py_kmer(M.seqs[s[0]], row_pos(s, int(r)), s[3]) for r in rows], s
    return got.tobytes(), pu.counters(), info


def case_alignment_sequences(M, R):
    """18. unc_align_pileup_call on stretches of sequences 2, 4 and 0, both strands: one round of 2 209 rows (three workgroups of
    k_pileup_accum that stride over eight alignments), and three rounds or more of the same, whose table is the same byte for byte"""
    one = aligned_pileup(M, R, None, 0)
    assert [int(x) for x in one[2]["n_rows"]] == MULTI_ROWS and not one[2]["row_first"].any()
    # bins that two alignments, of two workgroups, reach
    assert int(np.frombuffer(one[0], np.uint64).reshape(-1, 5)[:, 0].max()) >= 2
    three = aligned_pileup(M, R, None, MULTI_WS)
    assert three[:2] == one[:2]


def case_alignment_sequences_band_and_cut(M, R):
    """18, continued: within a band of 40; with rows that may be cut, in the batch of eight and in one query alone"""
    from uncalled_amd import capi
    band = aligned_pileup(M, R, capi.align_opts(band=40), 0)
    assert [int(x) for x in band[2]["n_rows"]] == MULTI_ROWS
    cut = aligned_pileup(M, R, sc._ev(subseq=1), 0)
    assert cut[2]["row_first"].any() or [int(x) for x in cut[2]["n_rows"]] != MULTI_ROWS
    qs, _ = multi_batch(M)
    pu = M.pileup()
    one = [(4, M.lens[4] - 300, M.lens[4], False)]
    _, segs, info = capi.align_ref_batch(M.refseq, R.raw, R.offsets, R.calib, qs[:1], one, sc._ev(subseq=1), segments=True, pileup=pu)
    assert int(info["row_first"][0]) > 0 or int(info["n_rows"][0]) < 296
    equals_naive_big(pu, naive_of_segments(every(M), one, segs, info))


def case_alignment_sequences_accumulator_and_regions(M, R):
    """18, continued: an accumulator and a pile-up in one call equal their runs alone (case 8, on a grid of three); with regions in
    sequence 2 only the rows of the stretches of sequences 4 and 0 are outside, all of them"""
    from uncalled_amd import capi
    qs, stretches = multi_batch(M)
    alone, pu_alone = capi.ModelAcc(lib=M.L), M.pileup()
    capi.align_ref_batch(M.refseq, R.raw, R.offsets, R.calib, qs, stretches, accumulate=alone)
    capi.align_ref_batch(M.refseq, R.raw, R.offsets, R.calib, qs, stretches, pileup=pu_alone)
    acc, pu = capi.ModelAcc(lib=M.L), M.pileup()
    res = capi.align_ref_batch(M.refseq, R.raw, R.offsets, R.calib, qs, stretches, accumulate=acc, pileup=pu)
    assert (res["status"] == capi.DTW_OK).all()
    assert all(np.array_equal(x, y) for x, y in zip(acc.read()[:4], alone.read()[:4])) and acc.read()[4] == alone.read()[4]
    assert int(acc.read()[0].sum()) > 1000
    assert table(pu).tobytes() == table(pu_alone).tobytes() and pu.counters() == pu_alone.counters() and pu.counters()[2] > 1000
    # sequence 2 in two regions that touch: the four k-mers that hang over the first one's end (positions 196..199, rows of stretch 0
    # only) are outside too
    regions = [(2, 200, M.lens[2]), (2, 0, 200)]
    pu = M.pileup(regions)
    _, segs, info = capi.align_ref_batch(M.refseq, R.raw, R.offsets, R.calib, qs, stretches, segments=True, pileup=pu)
    assert [int(x) for x in info["n_rows"]] == MULTI_ROWS and not info["row_first"].any()
    nv = naive_of_segments(regions, stretches, segs, info)
    others = sum(int((seg["shared"] == 0).sum()) for s, seg in zip(stretches, segs) if s[0] != 2)
    assert nv.outside == others + int((segs[0]["shared"][196:200] == 0).sum()) and 3 * 296 + 137 >= others > 800
    equals_naive_big(pu, nv)
    assert pu.counters()[1] == nv.outside

