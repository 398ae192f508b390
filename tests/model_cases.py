"""The cases of the pore model object and of the training accumulator, shared by tests/test_model_cpu.py (the lanesim emulator)
and tests/test_gpu_model.py (the MI355X).  L is the library under test (capi.load's handle).  The independent checkers:
tests/model_naive.py (Python integers) for the accumulator, tests/model_check.c (gcc, the same libm) for the three tables,
dtw_check.c and align_check.c, built with the model under test, for the alignment."""
import atexit
import ctypes as C
import shutil
import subprocess
import tempfile
from pathlib import Path

import numpy as np
import pytest

import model_naive as mn
import segments_cases as sc

HERE = Path(__file__).resolve().parent
ERR_ARG = -1
RECS_PER_BLOCK = 4096        # the kernel's grid rule (model_dev.h): one workgroup for every 4096 records
BASES = "ACGT"


def kmer_str(k):
    return "".join(BASES[(k >> (2 * (4 - b))) & 3] for b in range(5))


def random_pairs(seed):
    """means uniform in 40-140, stdvs in 0.5-5"""
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(40, 140, 1024), rng.uniform(0.5, 5, 1024)], axis=1).astype(np.float32)


def write_model(path, pairs, order=None, header="kmer\tlevel_mean\tlevel_stdv"):
    order = range(1024) if order is None else order
    with open(path, "w") as f:
        f.write(header + "\n")
        for k in order:
            f.write("%s\t%.9g\t%.9g\n" % (kmer_str(k), pairs[k][0], pairs[k][1]))


_check_lib = None


def check_tables(pairs, cmpl):
    """model_check.c -> (means, vars_x2, lognorm, model_mean, model_stdv)"""
    global _check_lib
    if _check_lib is None:
        tmp = tempfile.mkdtemp(prefix="model_check_")
        atexit.register(shutil.rmtree, tmp, ignore_errors=True)
        so = Path(tmp) / "libmodel_check.so"
        subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", str(so), str(HERE / "model_check.c"), "-lm"], check=True)
        _check_lib = C.CDLL(str(so))
        _check_lib.model_check_tables.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float)]
        _check_lib.model_check_tables.restype = None
    p = np.ascontiguousarray(pairs, np.float32)
    a, b, c = (np.empty(1024, np.float32) for _ in range(3))
    mm, ms = C.c_float(), C.c_float()
    _check_lib.model_check_tables(p.ctypes.data, 1 if cmpl else 0, a.ctypes.data, b.ctypes.data, c.ctypes.data, C.byref(mm), C.byref(ms))
    return a, b, c, mm.value, ms.value


def tables_equal(got, want):
    return all(np.asarray(g, np.float32).tobytes() == np.asarray(w, np.float32).tobytes() for g, w in zip(got, want))


# ------------------------------------------------------------------ the model object (no device)
def case_default_pairs(L):
    """1. the default model's pairs are those of r94_model_table.h"""
    import re
    from uncalled_amd import capi
    txt = (HERE.parent / "uncalled_amd" / "csrc" / "r94_model_table.h").read_text()
    bits = np.array([int(x, 16) for x in re.findall(r"0x([0-9A-Fa-f]{8})u", txt)], np.uint32)
    assert bits.size == 2048
    assert capi.Model.default(lib=L).pairs().tobytes() == bits.view(np.float32).tobytes()


def case_default_tables(L, index):
    """2. tables(cmpl=True) = the index's, tables(cmpl=False) = the DTW's, bit for bit"""
    from uncalled_amd import capi
    m = capi.Model.default(lib=L)
    assert tables_equal(m.tables(True), index.model_tables())
    assert tables_equal(m.tables(False)[:3], capi.dtw_model_tables(lib=L))
    tm, ts = C.c_float(), C.c_float()
    L.unc_align_model_target(C.byref(tm), C.byref(ts))
    assert m.tables(False)[3:] == (tm.value, ts.value)


def case_round_trip(L, tmp_path):
    """3. save, load: every bit of a random model.  4. a file in shuffled k-mer order loads equal"""
    from uncalled_amd import capi
    pairs = random_pairs(3)
    m = capi.Model.from_pairs(pairs, lib=L)
    assert m.pairs().tobytes() == pairs.tobytes()
    m.save(tmp_path / "m.txt")
    lines = (tmp_path / "m.txt").read_text().split("\n")
    assert lines[0] == "kmer\tlevel_mean\tlevel_stdv" and lines[1].startswith("AAAAA\t") and lines[1024].startswith("TTTTT\t") and len(lines) == 1026
    assert capi.Model.load(tmp_path / "m.txt", lib=L).pairs().tobytes() == pairs.tobytes()
    write_model(tmp_path / "s.txt", pairs, np.random.default_rng(4).permutation(1024), header="anything at all")
    back = capi.Model.load(tmp_path / "s.txt", lib=L)
    assert back.pairs().tobytes() == pairs.tobytes()
    assert tables_equal(back.tables(True), m.tables(True))


def case_malformed(L, tmp_path):
    """5. short, duplicate k-mer, bad k-mer string, stdv 0, NaN (and: missing file, something behind the last k-mer)"""
    from uncalled_amd import capi
    pairs = random_pairs(5)
    good = tmp_path / "good.txt"
    write_model(good, pairs)
    capi.Model.load(good, lib=L)
    rows = good.read_text().split("\n")[:-1]

    def refused(name, lines):
        (tmp_path / name).write_text("\n".join(lines) + "\n")
        h = C.c_void_p()
        rc = L.unc_model_load(str(tmp_path / name).encode(), C.byref(h))
        assert rc == ERR_ARG and not h.value, (name, rc)
        assert L.unc_last_error()

    refused("short.txt", rows[:1024])
    refused("dup.txt", rows[:7] + [rows[6]] + rows[8:])                       # AAACC twice, AAACG missing
    refused("badkmer.txt", rows[:9] + ["AANCA\t80\t2"] + rows[10:])
    refused("shortkmer.txt", rows[:9] + ["AACA\t80\t2"] + rows[10:])
    refused("stdv0.txt", rows[:20] + [rows[20].split("\t")[0] + "\t80\t0"] + rows[21:])
    refused("nan.txt", rows[:30] + [rows[30].split("\t")[0] + "\tnan\t2"] + rows[31:])
    refused("text.txt", rows[:30] + [rows[30].split("\t")[0] + "\tabc\t2"] + rows[31:])
    refused("more.txt", rows + ["AAAAA\t80\t2"])
    h = C.c_void_p()
    assert L.unc_model_load(str(tmp_path / "none.txt").encode(), C.byref(h)) != 0 and not h.value
    bad = pairs.copy()
    bad[17, 1] = -1.0
    assert L.unc_model_from_pairs(bad.ctypes.data, C.byref(h)) == ERR_ARG and not h.value


def case_random_tables(L):
    """6. the tables of a random model are model_check.c's, complemented and not"""
    from uncalled_amd import capi
    for seed in (6, 7):
        pairs = random_pairs(seed)
        m = capi.Model.from_pairs(pairs, lib=L)
        for cmpl in (True, False):
            assert tables_equal(m.tables(cmpl), check_tables(pairs, cmpl)), (seed, cmpl)
    d = capi.Model.default(lib=L)
    assert tables_equal(d.tables(True), check_tables(d.pairs(), True))


# ------------------------------------------------------------------ the accumulator through acc_add
def read_equals(acc, want):
    got = mn.of_read(acc.read())
    for f in ("n", "S", "SS"):
        bad = [k for k in range(1024) if got[f][k] != want[f][k]]
        assert not bad, (f, bad[:4], [got[f][k] for k in bad[:4]], [want[f][k] for k in bad[:4]])
    assert got["dropped"] == want["dropped"], (got["dropped"], want["dropped"])
    return got


def case_one_bin(L):
    """7. one k-mer, k-mer 0: every lane on one bin.  The grid is one workgroup for every 4096 records: 200 records are one workgroup
    (more than a wavefront's 64 lanes), 4096 + 200 are two, and both flush into bin 0"""
    from uncalled_amd import capi
    rng = np.random.default_rng(7)
    for n in (200, RECS_PER_BLOCK + 200):
        lv = rng.uniform(-100, 150, n).astype(np.float32)
        acc = capi.ModelAcc(lib=L)
        acc.add(np.zeros(n, np.uint16), lv)
        got = read_equals(acc, mn.accumulate(np.zeros(n, np.uint16), lv))
        assert got["n"][0] == n and sum(got["n"]) == n


def case_carry(L):
    """8. five records of 2047.5 into k-mer 1023: SS crosses 2^64, the high word is 1.  Negative levels: negative S"""
    from uncalled_amd import capi
    acc = capi.ModelAcc(lib=L)
    km = np.array([1023] * 5 + [5] * 3, np.uint16)
    lv = np.array([2047.5] * 5 + [-1000.25, -3.5, 1.0], np.float32)
    acc.add(km, lv)
    n, S, lo, hi, dropped = acc.read()
    assert int(hi[1023]) == 1 and int(n[1023]) == 5 and int(S[5]) < 0 and dropped == 0
    read_equals(acc, mn.accumulate(km, lv))
    # the carry out of the low word in GLOBAL memory: a second call adds to what the first left
    acc.add(km[:5], lv[:5])
    want = mn.accumulate(km[:5], lv[:5], into=mn.accumulate(km, lv))
    assert want["SS"][1023] >> 64 == 2
    read_equals(acc, want)


def case_drop_and_skip(L):
    """9. NaN, +inf, -inf, 2048 and -2048 are dropped and counted; 2047.999 is kept; shared = 1 is skipped without the flag, kept with"""
    from uncalled_amd import capi
    lv = np.array([np.nan, np.inf, -np.inf, 2048.0, -2048.0, 2047.999, -2047.999, 80.0, 90.0], np.float32)
    km = np.array([1, 2, 3, 4, 5, 6, 7, 8, 8], np.uint16)
    sh = np.array([0, 0, 0, 0, 0, 0, 0, 0, 1], np.uint32)
    for keep in (False, True):
        acc = capi.ModelAcc(keep_shared=keep, lib=L)
        acc.add(km, lv, sh)
        got = read_equals(acc, mn.accumulate(km, lv, sh, keep_shared=keep))
        assert got["dropped"] == 5 and got["n"][6] == 1 and got["n"][7] == 1 and got["n"][8] == (2 if keep else 1)
        assert sum(got["n"][1:6]) == 0
        acc.reset()
        assert mn.of_read(acc.read()) == mn.accumulate([], [])
    acc = capi.ModelAcc(lib=L)
    assert L.unc_model_acc_add(acc.h, 1, np.array([1024], np.uint16).ctypes.data, lv.ctypes.data, None, None) == ERR_ARG


def case_split_and_order(L):
    """10. 5 000 random records over all k-mers in one call, in 7 calls and reversed: three identical reads, equal to model_naive"""
    from uncalled_amd import capi
    rng = np.random.default_rng(10)
    n = 5000
    km = rng.integers(0, 1024, n).astype(np.uint16)
    km[:1024] = np.arange(1024)
    lv = (rng.standard_normal(n) * 300).astype(np.float32)
    sh = (rng.random(n) < 0.1).astype(np.uint32)
    want = mn.accumulate(km, lv, sh)
    one, seven, rev = (capi.ModelAcc(lib=L) for _ in range(3))
    one.add(km, lv, sh)
    for part in np.array_split(np.arange(n), 7):
        seven.add(km[part], lv[part], sh[part])
    rev.add(km[::-1], lv[::-1], sh[::-1])
    reads = [a.read() for a in (one, seven, rev)]
    for r in reads[1:]:
        assert all(np.array_equal(x, y) for x, y in zip(r[:4], reads[0][:4])) and r[4] == reads[0][4]
    read_equals(one, want)
    return one, want


def case_finish(L):
    """11. finish against model_naive in bits; a k-mer below min_obs, n = 1 and identical levels keep the prior's row"""
    from uncalled_amd import capi
    rng = np.random.default_rng(11)
    prior_pairs = random_pairs(12)
    prior = capi.Model.from_pairs(prior_pairs, lib=L)
    km = np.concatenate([np.full(1, 0), np.full(4, 1), np.full(6, 2), np.full(5, 3), rng.integers(4, 1024, 6000)]).astype(np.uint16)
    lv = np.concatenate([[70.0], rng.uniform(60, 90, 4), np.full(6, 81.25), rng.uniform(60, 90, 5),
                         rng.uniform(40, 140, 6000)]).astype(np.float32)
    acc = capi.ModelAcc(lib=L)
    acc.add(km, lv)
    naive = mn.accumulate(km, lv)
    for min_obs, prior_m, prior_p in ((5, prior, prior_pairs), (0, None, capi.Model.default(lib=L).pairs())):
        m, kept = acc.finish(prior_m, min_obs)
        want, want_kept = mn.finish(naive, prior_p, min_obs)
        got = m.pairs()
        assert got.tobytes() == want.tobytes(), np.argwhere(got != want)[:4]
        assert kept == want_kept
        assert got[0].tobytes() == prior_p[0].tobytes() and got[2].tobytes() == prior_p[2].tobytes()       # n = 1; V = 0
        assert (got[1].tobytes() == prior_p[1].tobytes()) == (min_obs == 5)                               # 4 records: below 5
        assert got[3].tobytes() != prior_p[3].tobytes() and kept >= 3
    # means and deviations near what the records have
    assert abs(float(got[3, 0]) - float(lv[11:16].astype(np.float64).mean())) < 1e-4


# ------------------------------------------------------------------ through the alignment
def batch(R):
    """case_rounds' six queries of segments_cases.py (50 rows on about 200 columns each) and a seventh on another read"""
    qs = [(0, 300 * i, 300 * i + 1000) for i in range(6)] + [(2, 0, 0)]
    kms = [R.walk[20 * i:20 * i + 50] for i in range(6)] + [R.walk[:60]]
    return qs, kms


def naive_of_segments(kms, segs, info, keep_shared=False):
    acc = None
    for km, s, inf in zip(kms, segs, info):
        assert s.size == int(inf["n_rows"])
        rows = km[int(inf["row_first"]):int(inf["row_first"]) + s.size]
        acc = mn.accumulate(rows, s["level"], s["shared"], keep_shared, into=acc)
    return acc


def case_align_accumulates(L, R):
    """12. segments and an accumulator in one call: model_naive over the returned records and k-mers equals read()
    13. seg == NULL; a workspace that forces three rounds or more; the queries permuted: identical accumulators"""
    from uncalled_amd import capi
    qs, kms = batch(R)
    for keep in (False, True):
        acc = capi.ModelAcc(keep_shared=keep, lib=L)
        res, segs, info = capi.align_batch(R.raw, R.offsets, R.calib, qs, kms, lib=L, segments=True, accumulate=acc)
        assert (res["status"] == capi.DTW_OK).all() and (info["status"] == capi.SEG_OK).all()
        want = naive_of_segments(kms, segs, info, keep)
        assert sum(want["n"]) > 300 and (keep or sum(want["n"]) < sum(int(x) for x in info["n_rows"]))
        first = read_equals(acc, want)
        plain = capi.align_batch(R.raw, R.offsets, R.calib, qs, kms, lib=L, segments=True)
        assert plain[0].tobytes() == res.tobytes() and all(sc.rec_equal(a, b) for a, b in zip(plain[1], segs))

        nul = capi.ModelAcc(keep_shared=keep, lib=L)
        res2 = capi.align_batch(R.raw, R.offsets, R.calib, qs, kms, lib=L, accumulate=nul)
        assert res2.tobytes() == res.tobytes()
        assert mn.of_read(nul.read()) == first

        rounds = capi.ModelAcc(keep_shared=keep, lib=L)
        res3 = capi.align_batch(R.raw, R.offsets, R.calib, qs, kms, lib=L, accumulate=rounds, workspace_bytes=6200)
        assert capi.dtw_last_timing(L)[1] >= 3 and (res3["status"] == capi.DTW_OK).all()
        assert mn.of_read(rounds.read()) == first

        perm = [4, 6, 0, 2, 5, 1, 3]
        shuffled = capi.ModelAcc(keep_shared=keep, lib=L)
        capi.align_batch(R.raw, R.offsets, R.calib, [qs[i] for i in perm], [kms[i] for i in perm], lib=L, accumulate=shuffled)
        assert mn.of_read(shuffled.read()) == first
    # a query without a path contributes nothing; the caller's short room in seg does not change what is summed
    o = capi.align_opts(max_events=80)
    acc = capi.ModelAcc(lib=L)
    res, segs, info = capi.align_batch(R.raw, R.offsets, R.calib, qs[:2] + [(0, 0, 300)], kms[:2] + [R.walk[:40]], o, lib=L, segments=True,
                                       accumulate=acc)
    assert list(res["status"]) == [capi.ALIGN_TOO_MANY, capi.ALIGN_TOO_MANY, capi.DTW_OK] and int(info["status"][0]) == capi.SEG_NONE
    read_equals(acc, naive_of_segments([kms[0], kms[1], R.walk[:40]], segs, info))


def case_align_short_room(L, R):
    """13 (the caller's room): seg with room for three records a query reports UNC_SEG_TRUNCATED and the accumulator holds them all"""
    from uncalled_amd import capi
    qs, kms = batch(R)
    full = capi.ModelAcc(lib=L)
    capi.align_batch(R.raw, R.offsets, R.calib, qs, kms, lib=L, accumulate=full)
    a = sc.call(L, R, qs, kms, seg_rooms=[3] * len(qs))
    assert a["rc"] == 0 and (a["info"]["status"] == capi.SEG_TRUNCATED).all()
    short = capi.ModelAcc(lib=L)
    n = len(qs)
    km = np.concatenate(kms + [np.zeros(1, np.uint16)])
    km_off = np.cumsum([0] + [k.size for k in kms]).astype(np.uint64)
    q = np.zeros(n, capi.ALIGN_QUERY)
    for i, (r, st, en) in enumerate(qs):
        q[i]["read"], q[i]["smp_st"], q[i]["smp_en"] = r, st, en
    res = np.zeros(n, capi.ALIGN_RESULT)
    seg = np.zeros(3 * n, capi.SEGMENT)
    seg_off = (3 * np.arange(n + 1)).astype(np.uint64)
    info = np.zeros(n, capi.SEG_INFO)
    so = capi.AlignSegments()
    so.seg, so.seg_off, so.info = seg.ctypes.data, seg_off.ctypes.data, info.ctypes.data
    rec = capi.AlignCall()
    rec.size = C.sizeof(capi.AlignCall)
    rec.n_reads, rec.raw, rec.offsets, rec.calib = len(R.signals), R.raw.ctypes.data, R.offsets.ctypes.data, R.calib.ctypes.data
    rec.n_queries, rec.queries, rec.kmers, rec.km_off, rec.results = n, q.ctypes.data, km.ctypes.data, km_off.ctypes.data, res.ctypes.data
    rec.segs = C.cast(C.pointer(so), C.c_void_p)
    rec.accumulate = short.h
    assert L.unc_align_call(C.byref(rec)) == 0, L.unc_last_error()
    assert (info["status"] == capi.SEG_TRUNCATED).all() and info.tobytes() == a["info"].tobytes()
    assert all(sc.rec_equal(seg[3 * i:3 * i + 3], a["segs"][i][:3]) for i in range(n))
    assert mn.of_read(short.read()) == mn.of_read(full.read())
    # the record's own checks
    rec.size = C.sizeof(capi.AlignCall) + 8
    assert L.unc_align_call(C.byref(rec)) == ERR_ARG
    rec.size = C.sizeof(capi.AlignCall)
    rec.kmers = None
    assert L.unc_align_call(C.byref(rec)) == ERR_ARG


def same_outputs(a, b):
    assert a[0].tobytes() == b[0].tobytes()
    for x, y in zip(a[1], b[1]):
        assert x.tobytes() == y.tobytes()
    for x, y in zip(a[2], b[2]):
        assert (x is None and y is None) or x.tobytes() == y.tobytes()
    assert all(sc.rec_equal(x, y) for x, y in zip(a[3], b[3])) and a[4].tobytes() == b[4].tobytes()


def case_default_model_changes_nothing(L, R):
    """14. results, levels, paths and records with model = Model.default() are those of the call without a model, byte for byte"""
    from uncalled_amd import capi
    qs, kms = batch(R)
    m = capi.Model.default(lib=L)
    for o in (None, capi.align_opts(target="model", band=40), sc._ev(subseq=2)):
        same_outputs(capi.align_batch(R.raw, R.offsets, R.calib, qs, kms, o, lib=L, levels=True, paths=True, segments=True, model=m),
                     capi.align_batch(R.raw, R.offsets, R.calib, qs, kms, o, lib=L, levels=True, paths=True, segments=True))


def model_chain(po, L, model):
    """segments_cases' checker chain with the checkers built for `model`"""
    from align_check import AlignChecker
    from dtw_check import Checker
    t = model.tables(False)
    ch = sc.Chain(po)
    ch.ac, ch.dc, ch.model_target = AlignChecker(model_means=t[0]), Checker(model=t[:3]), (t[3], t[4])
    return ch


def case_random_model_alignment(L, R, po):
    """15. with a random model, results, levels and paths equal the checker chain built with that model"""
    from uncalled_amd import capi
    model = capi.Model.from_pairs(random_pairs(15), lib=L)
    ch = model_chain(po, L, model)
    qs, kms = batch(R)
    qs, kms = qs[:3] + qs[6:], kms[:3] + kms[6:]
    differs = False
    for o in (None, capi.align_opts(target="model"), sc._ev(cost=0)):
        res, lev, paths, segs, info = capi.align_batch(R.raw, R.offsets, R.calib, qs, kms, o, lib=L, levels=True, paths=True, segments=True,
                                                       model=model)
        base = capi.align_batch(R.raw, R.offsets, R.calib, qs, kms, o, lib=L)
        differs |= base["dtw"]["score"].tobytes() != res["dtw"]["score"].tobytes()
        for q, ((r, st, en), km) in enumerate(zip(qs, kms)):
            e = ch.expected(R.signals[r], sc.CALIB, (st, en), km, o)
            assert int(res["status"][q]) == capi.DTW_OK
            assert lev[q].tobytes() == np.asarray(e["levels"], np.float32).tobytes(), q
            assert np.float32(res["scale"][q]) == np.float32(e["scale"]) and np.float32(res["shift"][q]) == np.float32(e["shift"])
            assert int(res["dtw"]["score"][q:q + 1].view(np.uint32)[0]) == e["dtw"]["score_bits"], q
            assert int(res["dtw"]["path_len"][q]) == e["dtw"]["path_len"] and np.array_equal(paths[q], e["dtw"]["path"]), q
            assert sc.rec_equal(segs[q], e["segs"]) and int(info["row_first"][q]) == e["row_first"]
    assert differs


def case_dtw_model_batch(L):
    """16. unc_dtw_model_batch on two hand-sized alignments, full and banded, against dtw_check.c built with the model"""
    from dtw_check import Checker
    from uncalled_amd import capi
    model = capi.Model.from_pairs(random_pairs(16), lib=L)
    t = model.tables(False)
    dc = Checker(model=t[:3])
    rng = np.random.default_rng(16)
    kms = [np.array([3, 700, 1023, 0, 512], np.uint16), rng.integers(0, 1024, 70).astype(np.uint16)]
    evs = [t[0][[3, 3, 700, 1023, 1023, 0, 512]] + np.float32(0.5), (t[0][np.repeat(kms[1], 2)] + rng.standard_normal(140)).astype(np.float32)]
    for cost in (capi.DTW_R94P, capi.DTW_R94D):
        prm = capi.DTWParams(capi.DTW_NONE, cost, 2.0, 1.0, 100.0)
        for band in (0, 1000):
            res, paths = capi.dtw_batch(evs, kms, prm, lib=L, full=True, band=band, model=model)
            base, _ = capi.dtw_batch(evs, kms, prm, lib=L, full=True, band=band)
            none, npaths = capi.dtw_batch(evs, kms, prm, lib=L, full=True, band=band, model=capi.Model.default(lib=L))
            assert none.tobytes() == base.tobytes() and res["score"].tobytes() != base["score"].tobytes()
            for a in range(2):
                e = dc.dtw(evs[a], kms[a], 0, cost, 2.0, 1.0, 100.0)
                assert int(res["score"][a:a + 1].view(np.uint32)[0]) == e["score_bits"] and np.array_equal(paths[a], e["path"]), (cost, band, a)
    bad = capi.DTWParams(capi.DTW_ROW, 1, 2.0, 1.0, 100.0)
    with pytest.raises(capi.UncalledHipError):
        capi.dtw_batch(evs, kms, bad, lib=L, band=8, model=model)


# ------------------------------------------------------------------ mapping
def case_set_model(L, example, goldens):
    """17. set_model(load(file written from the default)): the example read and the 48 parity reads of the fixture (sim_signal)
    map to hits identical to those of an index without set_model, and to the reference's own answers
    18. with a random model unc_match_probs over 16 levels is dtw_check_cost's formula over tables(cmpl=True)
    19. set_model once a mapper was made: UNC_ERR_ARG"""
    from dtw_check import Checker
    from uncalled_amd import capi
    from tools.simulate_reads import CAL_DIGITISATION, CAL_OFFSET, CAL_RANGE
    import tempfile as tf
    raw = example["signal"]
    off = np.array([0, raw.size], np.uint64)
    cal = capi.make_calib(1, example["range"], example["offset"], example["digitisation"])
    sim_off = np.ascontiguousarray(goldens["sim_offsets"], np.uint64)
    n_sim = sim_off.size - 1
    sim_raw = np.ascontiguousarray(goldens["sim_signal"][:int(sim_off[-1])], np.int16)
    sim_cal = capi.make_calib(n_sim, CAL_RANGE, CAL_OFFSET, CAL_DIGITISATION)
    plain = capi.Index(example["prefix"], lib=L)
    pm = capi.Mapper(plain, n_slots=4)
    want = pm.map_batch(raw, off, cal)
    want_sim = pm.map_batch(sim_raw, sim_off, sim_cal)
    assert int(want["mapped"][0]) == 1 and n_sim == 48 and int(want_sim["mapped"].sum()) > 24
    with tf.TemporaryDirectory() as d:
        capi.Model.default(lib=L).save(Path(d) / "r94.txt")
        loaded = capi.Model.load(Path(d) / "r94.txt", lib=L)
    ix = capi.Index(example["prefix"], lib=L)
    rnd = capi.Model.from_pairs(random_pairs(18), lib=L)
    ix.set_model(rnd)
    assert tables_equal(ix.model_tables(), rnd.tables(True)) and not tables_equal(ix.model_tables(), plain.model_tables())
    t = rnd.tables(True)
    dc = Checker(model=t[:3])
    levels = np.linspace(50, 130, 16).astype(np.float32)
    got = ix.match_probs(levels)
    want_probs = np.array([[-dc.cost(0, k, lv) for k in range(1024)] for lv in levels], np.float32)
    assert got.shape == (16, 1024) and got.tobytes() == want_probs.tobytes(), np.argwhere(got != want_probs)[:4]
    assert got.tobytes() != plain.match_probs(levels).tobytes()
    ix.set_model(loaded)
    assert tables_equal(ix.model_tables(), plain.model_tables())
    m = capi.Mapper(ix, n_slots=4)
    got = m.map_batch(raw, off, cal)
    got_sim = m.map_batch(sim_raw, sim_off, sim_cal)
    for f in capi.RESULT_FIELDS:
        assert got[f][0] == want[f][0], f
        assert np.array_equal(got_sim[f], want_sim[f]), f
    col = {str(n): j for j, n in enumerate(goldens["hit_fields"])}
    for name in ("mapped", "rd_st", "rd_en", "rd_len", "rf_st", "rf_en", "matches", "event_i", "n_nbr", "n_lf"):
        assert [int(x) for x in got_sim[name]] == [int(goldens["sim_hits"][i][col[name]]) for i in range(n_sim)], name
    assert L.unc_index_set_model(ix.h, rnd.h) == ERR_ARG and b"mapper" in L.unc_last_error()
    assert tables_equal(ix.model_tables(), plain.model_tables())
