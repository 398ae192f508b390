"""TEST INFRASTRUCTURE shared by tests/test_refalign_cpu.py (k_refseq.hip and unc_refseq.cpp under the lanesim emulator) and
tests/test_gpu_refalign.py (the gfx950 library): the packed reference on the device.

K-mers: unc_refseq_kmers_batch against unc_ref_kmers (the host function, the yardstick) for the same stretch, exact equality, and on
the tiny references also against py_kmers, a restatement from the FASTA string.
Alignment: unc_align_ref_batch against unc_align_batch fed unc_ref_kmers' output, both called through the C ABI into buffers full of
sentinels that are then compared whole: every byte of every result record, of the levels, of the paths and of what lies around them."""
import ctypes as C

import numpy as np

LENGTHS = (0, 4, 5, 6, 8, 9, 20, 21, 63, 64, 65, 68, 69, 127, 128, 129, 133)
KM_SENTINEL = 0xBEEF            # no k-mer: they are below 1024
ERR_ARG, ERR_IO = -1, -2


# ------------------------------------------------------------------ k-mers
def py_kmers(seq, st, en, fwd):
    """BwaIndex::get_kmers from the FASTA string: the 5-mers of seq[st:en], first base in the top bits; the minus strand's are the
    5-mers of the reverse complement"""
    s = seq[st:en]
    if not fwd:
        s = s[::-1].translate(str.maketrans("ACGT", "TGCA"))
    code = {"A": 0, "C": 1, "G": 2, "T": 3}
    return np.array([sum(code[c] << (2 * (4 - i)) for i, c in enumerate(s[j:j + 5])) for j in range(max(0, len(s) - 4))], np.uint16)


def tiny_reference(tmp_path, m, seed=5):
    """three sequences without N, l_pac % 4 == m; the second and the third start at offsets 141 and 291, no multiples of 4
    -> (prefix, [sequence strings])"""
    from uncalled_amd import build_index
    rng = np.random.default_rng(seed + m)
    lens = (141, 150, 145 + m)
    assert sum(lens) % 4 == m and lens[0] % 4 and (lens[0] + lens[1]) % 4
    seqs = ["".join("ACGT"[b] for b in rng.integers(0, 4, n)) for n in lens]
    fa = tmp_path / ("tiny%d.fa" % m)
    fa.write_text("".join(">t%d\n%s\n" % (i, s) for i, s in enumerate(seqs)))
    prefix = str(tmp_path / ("tiny%d" % m))
    build_index.build_from_fasta(str(fa), prefix)
    return prefix, seqs


MULTI_LENS = (141, 4, 131075, 150, 132703)
MULTI_BINS = 528106            # 2 * (137 + 0 + 131071 + 146 + 132699): the default pile-up's table, 516 workgroups of the covered-bin kernels


def multi_reference(tmp_path, seed=7):
    """five sequences without N: the second is shorter than a k-mer, the third and the fifth start at offsets 145 and 131370, no
    multiples of 4, and the default pile-up's table takes k_pileup_scan three passes -> (prefix, [sequence strings])"""
    from uncalled_amd import build_index
    rng = np.random.default_rng(seed)
    lens = MULTI_LENS
    assert sum(lens[:2]) % 4 and sum(lens[:4]) % 4 and lens[1] < 5
    assert 2 * sum(max(0, n - 4) for n in lens) == MULTI_BINS and -(-MULTI_BINS // 1024) == 516 > 2 * 256
    seqs = ["".join(np.array(list("ACGT"))[rng.integers(0, 4, n)]) for n in lens]
    fa = tmp_path / "multi.fa"
    fa.write_text("".join(">m%d\n%s\n" % (i, s) for i, s in enumerate(seqs)))
    prefix = str(tmp_path / "multi")
    build_index.build_from_fasta(str(fa), prefix)
    return prefix, seqs


def random_reference(tmp_path, n_bases, seed=6, name="long"):
    from uncalled_amd import build_index
    rng = np.random.default_rng(seed)
    seq = "".join(np.array(list("ACGT"))[rng.integers(0, 4, n_bases)])
    fa = tmp_path / (name + ".fa")
    fa.write_text(">%s\n%s\n" % (name, seq))
    prefix = str(tmp_path / name)
    build_index.build_from_fasta(str(fa), prefix)
    return prefix, [seq]


def tiny_stretches(seq_lens):
    """per sequence: every st in 0..8 x every length of LENGTHS that fits x both strands, and every length ending at the
    sequence's last base (the last sequence's is l_pac's)"""
    out = []
    for rid, n in enumerate(seq_lens):
        for fwd in (True, False):
            for ln in LENGTHS:
                out += [(rid, st, st + ln, fwd) for st in range(9) if st + ln <= n]
                out.append((rid, n - ln, n, fwd))
    return out


def kmers_batch_raw(refseq, stretches, gaps=(0, 1, 3, 8, 5, 2, 16, 7), lead=3):
    """unc_refseq_kmers_batch into an array of sentinels, stretch a's room its count plus a gap -> (rc, out, out_off, counts)"""
    from uncalled_amd import capi
    ss = capi._stretches(stretches)
    counts = [max(0, en - st - 4) for _, st, en, _ in stretches]
    off = (lead + np.cumsum([0] + [c + gaps[a % len(gaps)] for a, c in enumerate(counts)])).astype(np.uint64)
    out = np.full(int(off[-1]) + 11, KM_SENTINEL, np.uint16)
    rc = refseq.L.unc_refseq_kmers_batch(refseq.h, len(stretches), ss.ctypes.data, out.ctypes.data, off.ctypes.data, None)
    return rc, out, off, counts


def check_kmers(refseq, index, prefix, stretches, seqs=None):
    """one call for all stretches; every stretch equals unc_ref_kmers (and py_kmers, given the sequences), and every word outside
    the counts still holds the sentinel -> k-mers compared"""
    from uncalled_amd import capi
    rc, out, off, counts = kmers_batch_raw(refseq, stretches)
    assert rc == 0, refseq.L.unc_last_error()
    written = np.zeros(out.size, bool)
    for a, (rid, st, en, fwd) in enumerate(stretches):
        got = out[int(off[a]):int(off[a]) + counts[a]]
        want = capi.ref_kmers(index, prefix, rid, st, en, fwd)
        assert want.size == counts[a] and np.array_equal(got, want), (a, rid, st, en, fwd)
        if seqs is not None:
            assert np.array_equal(got, py_kmers(seqs[rid], st, en, fwd)), (a, rid, st, en, fwd)
        written[int(off[a]):int(off[a]) + counts[a]] = True
    assert (out[~written] == KM_SENTINEL).all()
    return int(sum(counts))


def check_loader(index, prefix, tmp_path):
    """a .pac one byte short, one byte long, with a wrong tail byte, missing: UNC_ERR_IO each, the file's name in the message"""
    import os
    L = index.L
    good = open(prefix + ".pac", "rb").read()
    l_pac = L.unc_index_size(index.h) // 2
    assert len(good) == l_pac // 4 + 2 and good[-1] == l_pac % 4
    bad = str(tmp_path / "bad")
    for what, data in (("short", good[:-1]), ("long", good + b"\0"), ("tail", good[:-1] + bytes([(good[-1] + 1) % 4])), ("missing", None)):
        if data is None:
            os.unlink(bad + ".pac")
        else:
            open(bad + ".pac", "wb").write(data)
        h = C.c_void_p()
        rc = L.unc_refseq_load(index.h, bad.encode(), C.byref(h))
        assert rc == ERR_IO and not h.value and b"bad.pac" in L.unc_last_error(), (what, rc, L.unc_last_error())


def check_kmer_argument_errors(refseq, seq_lens):
    """rid out of range, st > en, en past the sequence, room smaller than the count, descending offsets: UNC_ERR_ARG, out untouched"""
    from uncalled_amd import capi
    L = refseq.L
    ok = (0, 0, 30, True)
    for bad in ((-1, 0, 30, True), (len(seq_lens), 0, 30, True), (0, 31, 30, True), (0, 0, seq_lens[0] + 1, False),
                (len(seq_lens) - 1, 5, seq_lens[-1] + 1, True)):
        rc, out, _, _ = kmers_batch_raw(refseq, [ok, bad, ok])
        assert rc == ERR_ARG and (out == KM_SENTINEL).all(), bad
    ss = capi._stretches([ok, ok])
    out = np.full(80, KM_SENTINEL, np.uint16)
    for off in ([0, 26, 51], [0, 25, 52], [30, 0, 30], [0, 30, 29]):      # 26 k-mers each
        o = np.array(off, np.uint64)
        rc = L.unc_refseq_kmers_batch(refseq.h, 2, ss.ctypes.data, out.ctypes.data, o.ctypes.data, None)
        assert rc == ERR_ARG and (out == KM_SENTINEL).all(), off
    assert L.unc_refseq_kmers_batch(refseq.h, 0, None, None, None, None) == 0       # no stretches: nothing to do
    rc, out, off, counts = kmers_batch_raw(refseq, [(0, 3, 7, True), (0, 0, 0, False)])      # below five bases: legal, nothing written
    assert rc == 0 and counts == [0, 0] and (out == KM_SENTINEL).all()


# ------------------------------------------------------------------ the alignment contract
F32_SENTINEL = np.float32(-12345.5)
U32_SENTINEL = 0xA5A5A5A5


def golden_stretches(G, members, seq_len, fwd=None):
    """a stretch of the example reference per golden query: as many k-mers as the golden has, at a start that moves with the case;
    fwd None: the strands alternate"""
    out = []
    for c in members:
        n = int(G.kmers(c).size)
        st = (997 * c) % (seq_len - n - 4 + 1)
        out.append((0, st, st + n + 4, bool(c & 1) if fwd is None else fwd))
    return out


def run_both(G, refseq, index, prefix, queries, stretches, opts=None, workspace=0, path_rooms="full", kmers=True, stream=None):
    """unc_align_ref_batch and unc_align_batch (fed capi.ref_kmers) on the same queries; asserts that results, levels, paths and their
    surroundings are equal byte for byte and that kmers_out holds ref_kmers' output -> (results, rc).  With a return code other than
    0 both must give it and leave every buffer as it was."""
    from uncalled_amd import capi
    L = refseq.L
    n = len(queries)
    qs = np.zeros(n, capi.ALIGN_QUERY)
    for i, (r, st, en) in enumerate(queries):
        qs[i]["read"], qs[i]["smp_st"], qs[i]["smp_en"] = r, st, en
    kms = [capi.ref_kmers(index, prefix, *s) for s in stretches]
    km_off = np.cumsum([0] + [k.size for k in kms]).astype(np.uint64)
    km = np.concatenate(kms + [np.zeros(1, np.uint16)])
    ss = capi._stretches(stretches)
    raw_mode = opts is not None and opts.flags & capi.ALIGN_RAW
    room = []
    for r, st, en in queries:
        ln = int(G.offsets[r + 1] - G.offsets[r]) if r < len(G.offsets) - 1 else 0       # (a bad query is the library's to refuse)
        ns = max(0, (int(en) if en else ln) - int(st))
        room.append(ns if raw_mode else ns // 2 + 16)
    lev_off = np.cumsum([0] + room).astype(np.uint64)
    if path_rooms == "full":
        path_rooms = [c + k.size - 1 for c, k in zip(room, kms)]
    path_off = None if path_rooms is None else (2 + np.cumsum([0] + list(path_rooms))).astype(np.uint64)
    got = []
    for which in ("ref", "old"):
        res = np.full(n, 0xAB, np.uint8).repeat(capi.ALIGN_RESULT.itemsize).view(capi.ALIGN_RESULT)
        lev = np.full(int(lev_off[-1]) + 5, F32_SENTINEL, np.float32)
        path = None if path_off is None else np.full((int(path_off[-1]) + 5, 2), U32_SENTINEL, np.uint32)
        common = (int(workspace), res.ctypes.data, lev.ctypes.data, lev_off.ctypes.data)
        tail = (path.ctypes.data if path is not None else None, path_off.ctypes.data if path is not None else None, stream)
        head = (C.byref(opts) if opts is not None else None, len(G.offsets) - 1, G.raw.ctypes.data, G.offsets.ctypes.data, G.calib.ctypes.data, 0, n,
                qs.ctypes.data)
        if which == "ref":
            kout = np.full(int(km_off[-1]) + 4, KM_SENTINEL, np.uint16)
            rc = L.unc_align_ref_batch(refseq.h, None, *head, ss.ctypes.data, *common, kout.ctypes.data if kmers else None,
                                       km_off.ctypes.data if kmers else None, *tail)
            if rc == 0 and kmers:
                assert np.array_equal(kout[:int(km_off[-1])], km[:-1]) and (kout[int(km_off[-1]):] == KM_SENTINEL).all()
            else:
                assert (kout == KM_SENTINEL).all()
        else:
            rc = L.unc_align_batch(0, None, *head, km.ctypes.data, km_off.ctypes.data, *common, *tail)
        got.append((rc, res, lev, path))
    (rc, res, lev, path), (rc0, res0, lev0, path0) = got
    assert rc == rc0, (rc, rc0, L.unc_last_error())
    assert res.tobytes() == res0.tobytes()
    assert lev.tobytes() == lev0.tobytes()
    assert path is None or path.tobytes() == path0.tobytes()
    if rc != 0:
        assert (res.view(np.uint8) == 0xAB).all() and (lev == F32_SENTINEL).all() and (path is None or (path == U32_SENTINEL).all())
    return res, rc


def contract_cases(G, seq_len, small):
    """(name, members, stretches, opts, keywords of run_both, statuses that must occur) -- the cases of the contract.  small: the
    emulator's versions, without the example read's 31 668 samples"""
    from uncalled_amd import capi
    NONE, ROW, COL, R94P, R94D = capi.DTW_NONE, capi.DTW_ROW, capi.DTW_COL, capi.DTW_R94P, capi.DTW_R94D
    every = [c for c in range(G.n) if not small or G.signals[G.query(c)[0]].size < 20000]
    short = [c for c in every if 0 < G.query(c)[2] - G.query(c)[1] <= 2000]
    gs = lambda m, fwd=None: golden_stretches(G, m, seq_len, fwd)      # noqa: E731
    idx = G.idx
    narrow = [idx(n) for n in ("events_50", "events_12", "few_hundred", "events_1")]
    narrow_st = [(0, 100, 154, True), (0, 200, 304, False), (0, 300, 504, True), (0, 400, 407, False)]      # 100 rows on 12 columns
    many = [idx(n) for n in ("events_50", "events_0", "events_26", "all_masked", "events_25", "stalls")]
    one_read_q = [(0, 0, 0), (0, 100, 900), (0, 101, 1900), (0, 4000, 0)]
    cases = [
        ("as they stand", every, gs(every), capi.align_opts(), {}, {capi.DTW_OK, capi.ALIGN_NO_COLUMNS}),
        ("the minus strand", every, gs(every, False), capi.align_opts(), {}, {capi.DTW_OK}),
        ("one read, four queries", one_read_q, [(0, 50, 200, True), (0, 60, 180, False), (0, 9000, 9300, True), (0, 0, 90, False)],
         capi.align_opts(), {}, {capi.DTW_OK}),
        ("samples for columns", short, gs(short), capi.align_opts(create_events=False), {}, {capi.DTW_OK}),
        ("no mask", every, gs(every), capi.align_opts(mask=False), {}, {capi.DTW_OK}),
        ("the model's target", every, gs(every), capi.align_opts(target="model"), {}, {capi.DTW_OK}),
        ("rows may be cut", every, gs(every), capi.align_opts(dtw=capi.DTWParams(ROW, R94D, 2, 1, 100)), {}, {capi.DTW_OK}),
        ("columns may be cut", every, gs(every), capi.align_opts(dtw=capi.DTWParams(COL, R94P, 2, 1, 100)), {}, {capi.DTW_OK}),
        ("a band that binds", every, gs(every), capi.align_opts(band=4), {}, {capi.DTW_OK}),
        ("a band of all rows", every, gs(every), capi.align_opts(band=1 << 20), {}, {capi.DTW_OK}),
        ("too many events", many, gs(many), capi.align_opts(max_events=26), {}, {capi.ALIGN_TOO_MANY, capi.ALIGN_NO_COLUMNS, capi.DTW_OK}),
        ("a band too narrow", narrow, narrow_st, capi.align_opts(band=1), {}, {capi.DTW_BAND_TOO_NARROW, capi.DTW_OK}),
        ("two rounds", every, gs(every), capi.align_opts(), dict(workspace=200000), {capi.DTW_OK}),
        ("short rooms for the paths", short, gs(short), capi.align_opts(), dict(path_rooms=[(7 * a) % 40 for a in range(len(short))]),
         {capi.DTW_PATH_TRUNCATED}),
        ("no paths, no k-mers out", every, gs(every), capi.align_opts(), dict(path_rooms=None, kmers=False), {capi.DTW_OK}),
    ]
    out = []
    for name, members, stretches, opts, kw, statuses in cases:
        queries = members if isinstance(members[0], tuple) else [G.query(c) for c in members]
        out.append((name, queries, stretches, opts, kw, statuses))
    return out


def check_contract(G, refseq, index, prefix, seq_len, small):
    from uncalled_amd import capi
    seen = 0
    for name, queries, stretches, opts, kw, statuses in contract_cases(G, seq_len, small):
        res, rc = run_both(G, refseq, index, prefix, queries, stretches, opts, **kw)
        assert rc == 0, (name, refseq.L.unc_last_error())
        assert statuses <= set(map(int, res["status"])), (name, statuses, sorted(set(map(int, res["status"]))))
        if name == "two rounds":
            assert capi.dtw_last_timing(refseq.L)[1] >= 2
        seen += len(queries)
    return seen


def refused_stretch(G, refseq, good_s, s):
    """unc_align_ref_batch on a good stretch and on s: UNC_ERR_ARG and no result written; a stretch below five bases is named"""
    from uncalled_amd import capi
    L = refseq.L
    res = np.full(2, 0xAB, np.uint8).repeat(capi.ALIGN_RESULT.itemsize).view(capi.ALIGN_RESULT)
    qs = np.zeros(2, capi.ALIGN_QUERY)
    qs["read"], qs["smp_st"], qs["smp_en"] = 0, 1000, 1400
    ss = capi._stretches([good_s, s])
    rc = L.unc_align_ref_batch(refseq.h, None, None, len(G.offsets) - 1, G.raw.ctypes.data, G.offsets.ctypes.data, G.calib.ctypes.data, 0, 2,
                               qs.ctypes.data, ss.ctypes.data, 0, res.ctypes.data, None, None, None, None, None, None, None)
    assert rc == ERR_ARG and (res.view(np.uint8) == 0xAB).all(), s
    if s[2] - s[1] < 5 and s[1] <= s[2]:
        assert b"query 1 has no k-mers" in L.unc_last_error()


def multi_stretches(G, members, lens):
    """a stretch per golden query on multi_reference's sequences 0, 2, 3 and 4 in turn, as many k-mers as the golden has (the whole
    sequence where it holds fewer); per sequence the stretches start at its first base, end at its last and lie between, on both strands"""
    out = []
    for i, c in enumerate(members):
        rid = (0, 2, 3, 4)[i % 4]
        n = min(int(G.kmers(c).size) + 4, lens[rid])
        st = (0, lens[rid] - n, (997 * c) % (lens[rid] - n + 1))[(i // 4) % 3]
        out.append((rid, st, st + n, bool((i // 4) & 1)))
    return out


def check_multi(G, refseq, index, prefix, lens, small):
    """19. the alignment contract on sequences behind the first: unc_align_ref_batch against unc_align_batch fed unc_ref_kmers' output
    (run_both: every byte of results, levels, paths and what lies around them) for stretches on sequences 0, 2, 3 and 4, both strands;
    among them every such sequence's first five bases, its last five, and the two short sequences whole.  A stretch in the sequence of
    4 bases has no k-mers and rid == 5 names no sequence: refused, nothing written -> queries compared"""
    from uncalled_amd import capi
    assert list(lens) == list(MULTI_LENS)
    every = [c for c in range(G.n) if not small or G.signals[G.query(c)[0]].size < 20000]
    stretches = multi_stretches(G, every, lens)
    assert {(s[0], s[3]) for s in stretches} == {(r, f) for r in (0, 2, 3, 4) for f in (True, False)}
    assert {s[0] for s in stretches if s[1] == 0} == {0, 2, 3, 4} == {s[0] for s in stretches if s[2] == lens[s[0]]}
    queries = [G.query(c) for c in every]
    short = G.query(G.idx("events_50"))
    for rid in (0, 2, 3, 4):
        for fwd in (True, False):
            stretches += [(rid, 0, 5, fwd), (rid, lens[rid] - 5, lens[rid], fwd)] + ([(rid, 0, lens[rid], fwd)] if lens[rid] < 200 else [])
    queries += [short] * (len(stretches) - len(queries))
    seen = 0
    for opts, kw in ((capi.align_opts(), {}), (capi.align_opts(dtw=capi.DTWParams(capi.DTW_ROW, capi.DTW_R94D, 2, 1, 100)), {}),
                     (capi.align_opts(band=1 << 20), dict(workspace=200000))):
        res, rc = run_both(G, refseq, index, prefix, queries, stretches, opts, **kw)
        assert rc == 0, refseq.L.unc_last_error()
        assert capi.DTW_OK in set(map(int, res["status"])) and int((res["status"] == capi.DTW_OK).sum()) > len(queries) // 2
        seen += len(queries)
    assert capi.dtw_last_timing(refseq.L)[1] >= 2
    good_s = (2, 100, 144, True)
    for s in ((1, 0, 4, True), (1, 0, 4, False), (5, 0, 30, True), (3, 0, 151, True), (2, lens[2] - 10, lens[2] + 1, False)):
        refused_stretch(G, refseq, good_s, s)
    return seen


def check_align_argument_errors(G, refseq, index, prefix, seq_len):
    """what unc_align_batch refuses, and the stretches unc_refseq_kmers_batch refuses, and a stretch of four bases: UNC_ERR_ARG
    before any result is written"""
    from uncalled_amd import capi
    good_q, good_s = (0, 1000, 1400), (0, 100, 144, True)
    n0 = G.signals[0].size
    for q in ((0, 0, n0 + 1), (0, 200, 100), (len(G.signals), 0, 0)):       # both entry points refuse these, with the same code
        res, rc = run_both(G, refseq, index, prefix, [good_q, q], [good_s, good_s])
        assert rc == ERR_ARG, q
    for s in ((1, 100, 144, True), (-1, 100, 144, True), (0, 144, 100, True), (0, 100, seq_len + 1, False), (0, 100, 104, True), (0, 7, 7, False)):
        refused_stretch(G, refseq, good_s, s)
    # opts the pipeline refuses, through the binding
    import pytest
    for o in (capi.align_opts(dtw=capi.DTWParams(3, 0, 1, 1, 1)), capi.align_opts(dtw=capi.DTWParams(capi.DTW_ROW, 0, 1, 1, 1), band=3)):
        with pytest.raises(capi.UncalledHipError, match="error -1"):
            capi.align_ref_batch(refseq, G.raw, G.offsets, G.calib, [good_q], [good_s], opts=o)
