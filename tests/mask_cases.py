"""The cases of repeat masking shared by tests/test_mask_cpu.py (k_mask.hip under the emulator) and tests/test_gpu_mask.py (on the
GPU): every count, per-iteration report, final code and external count tap is compared for exact equality with tests/mask_naive.py.
The inputs are the smallest at which each kernel can go wrong; a lane of k_kmer_count / k_mask_flag_kmer owns 16 window starts
(mask_dev.h: MASK_RUN), a wavefront 1024, a lane of k_mask_cover 64 positions."""
import os

import numpy as np

import mask_naive as mn

LANE_RUN = 16


def rand_bases(rng, n, alphabet="ACGT"):
    return "".join(alphabet[i] for i in rng.integers(0, len(alphabet), n))


def revcomp(s):
    return "".join(mn.COMP[ch] for ch in reversed(s))


def offsets(contigs):
    return np.cumsum([0] + [len(s) for s in contigs]).astype(np.uint64)


def masker(capi, contigs, lib):
    return capi.Masker(np.array(mn.codes_of(contigs), dtype=np.uint8), offsets(contigs), lib=lib)


# ------------------------------------------------------------------------------------------------ internal masking
def internal_cases():
    rng = np.random.default_rng(20250)
    c = []
    # overlap
    c.append(dict(name="poly-A", contigs=["A" * 40], k=3, iters=1, report=[("AAA", 38, 40)]))
    c.append(dict(name="stride 2", contigs=["AC" * 20], k=4, iters=1, report=[("ACAC", 19, 40)]))
    c.append(dict(name="adjacent to itself", contigs=["ACGTACGTTTGCA"], k=4, iters=1, report=[("ACGT", 2, 8)]))
    # edges: a contig of exactly k bases, one of k - 1, an empty one, an occurrence ending at a contig's last base, a would-be
    # occurrence spanning two contigs, N and lower-case runs inside and at the ends, a window one base short of an N
    c.append(dict(name="edges", contigs=["ACG", "AC", "", "TTGACG", "TTAC", "GTT", "NNacgNNACGnACGN", "acN", "N", "nnnn", ""], k=3, iters=1,
                  report=[("ACG", 5, 15)]))
    # ties: the smaller code first, the other one in the next iteration; then nothing occurs twice: 2 of 5 iterations done
    c.append(dict(name="ties and the early stop", contigs=["TTTTT", "GGGGG", "ACGTCA"], k=3, iters=5,
                  report=[("GGG", 3, 5), ("TTT", 3, 5)]))
    c.append(dict(name="nothing twice", contigs=["ACGT"], k=2, iters=3, report=[]))
    c.append(dict(name="k = 1", contigs=["ACGTNAAcc", "t"], k=1, iters=3, report=[("A", 3, 3), ("C", 3, 3), ("T", 2, 2)]))
    # k = 13: 64 Mi counters; the tap is compared sparsely
    unit = rand_bases(rng, 13)
    c.append(dict(name="k = 13", contigs=[rand_bases(rng, 150) + unit + rand_bases(rng, 70) + unit + "N" + unit, unit[:12]], k=13, iters=2))
    # windows per text at the hand-overs: one lane's run, one wavefront's, a word of the cover kernel -- minus one, exactly, plus one
    for w in (LANE_RUN - 1, LANE_RUN, LANE_RUN + 1, 63, 64, 65, 64 * LANE_RUN - 1, 64 * LANE_RUN, 64 * LANE_RUN + 1):
        c.append(dict(name="%d windows" % w, contigs=[rand_bases(rng, w + 2, "AC")], k=3, iters=2))
        c.append(dict(name="%d windows, tail repeat" % w, contigs=[rand_bases(rng, w - 3, "ACGT") + "GGGGG"], k=3, iters=1))
    # several workgroups: grid stride, lane runs, hand-over between lanes and wavefronts, and the hot-counter path
    body = rand_bases(rng, 70000)
    tenmer = "GATTACAGCT"
    parts, at = [], 0
    for p in sorted(int(x) for x in rng.integers(0, 57000, 40)):
        parts.append(body[at:p] + tenmer)
        at = p
    big = "".join(parts) + body[at:58000]
    big = big[:35000] + "A" * 12000 + big[35000:]
    c.append(dict(name="several workgroups", contigs=[big[:30011], big[30011:], "N" * 700 + tenmer * 3], k=10, iters=3))
    return c


def check_internal(capi, case, lib=None):
    """counts before, the loop's report, the codes after and the counts after against the checker"""
    contigs, k, iters = case["contigs"], case["k"], case["iters"]
    want_contigs, want_report = mn.mask_internal(contigs, k, iters)
    if "report" in case:
        assert want_report == case["report"], (case["name"], want_report)
    with masker(capi, contigs, lib) as m:
        check_counts(m, contigs, k, case["name"])
        got = m.internal(k, iters)
        assert [(mn.kmer_code(kmer), occ, bases) for kmer, occ, bases in want_report] == got, (case["name"], want_report, got)
        codes = m.codes()
        assert codes.tolist() == mn.codes_of(want_contigs), case["name"]
        check_counts(m, want_contigs, k, case["name"])
    return want_report


def check_counts(m, contigs, k, name):
    want = mn.kmer_counts(contigs, k)
    got = m.kmer_counts(k)
    assert got.size == 4 ** k
    # (sparse: the checker's dictionary entry by entry, and nothing else is set)
    assert int(np.count_nonzero(got)) == len(want) and int(got.sum(dtype=np.uint64)) == sum(want.values()), name
    for kmer, cnt in want.items():
        assert int(got[mn.kmer_code(kmer)]) == cnt, (name, kmer)


def check_arguments(capi, lib=None):
    import pytest
    codes, off = np.zeros(8, np.uint8), np.array([0, 8], np.uint64)
    err = dict(match="error -1")
    with pytest.raises(capi.UncalledHipError, **err):
        capi.Masker(codes, np.array([0, 5, 3, 8], np.uint64), lib=lib)            # descending offsets
    with pytest.raises(capi.UncalledHipError, **err):
        capi.Masker(codes, np.array([0, 7], np.uint64), lib=lib)                  # offsets that do not end at n
    with pytest.raises(capi.UncalledHipError, **err):
        capi.Masker(codes, np.array([1, 8], np.uint64), lib=lib)
    L = lib or capi.load()
    h = capi.C.c_void_p()
    assert L.unc_mask_create(0, codes.ctypes.data, 1 << 32, off.ctypes.data, 1, capi.C.byref(h)) == -1 and not h.value    # n too large
    assert b"2^32" in L.unc_last_error()
    with capi.Masker(codes, off, lib=lib) as m:
        for k in (0, 14, 1 << 31):
            with pytest.raises(capi.UncalledHipError, **err):
                m.kmer_counts(k)
            with pytest.raises(capi.UncalledHipError, **err):
                m.internal(k, 1)
        with pytest.raises(capi.UncalledHipError, **err):
            m.internal(3, 0)
        assert m.codes().tolist() == [0] * 8


def check_lifecycle(capi, lib=None):
    """a masker freed and created again, and an empty one"""
    for _ in range(2):
        m = masker(capi, ["A" * 40], lib)
        assert m.internal(3, 2) == [(0, 38, 40)]
        assert m.codes().tolist() == [4] * 40
        m.close()
        m.close()
    # a million iterations asked of a loop that ends after two: the host stops queueing at the end of the first batch
    with masker(capi, ["TTTTT", "GGGGG", "ACGTCA"], lib) as m:
        assert m.internal(3, 1000000) == [(mn.kmer_code("GGG"), 3, 5), (mn.kmer_code("TTT"), 3, 5)]
    # more iterations done than one batch holds (32): 40 distinct 4-mers twice each, none overlapping another
    kmers = ["".join(mn.BASES[(i >> s) & 3] for s in (4, 2, 0)) + "A" for i in range(40)]
    with masker(capi, [km + "N" + km for km in kmers], lib) as m:
        got = m.internal(4, 50)
        assert got == [(mn.kmer_code(km), 2, 8) for km in sorted(kmers, key=mn.kmer_code)] and len(got) == 40
    with capi.Masker(np.zeros(0, np.uint8), np.array([0, 0, 0], np.uint64), lib=lib) as m:
        assert m.internal(3, 2) == [] and m.codes().size == 0 and int(m.kmer_counts(2).sum()) == 0


# ------------------------------------------------------------------------------------------------ external masking
def tiny_reference():
    """about 3 kb in two contigs: a 120-base segment in 1, 2 and 6 copies (one of the six reverse-complemented), a palindromic
    50-mer, an N-run, a lower-case run"""
    rng = np.random.default_rng(77)
    r = lambda n: rand_bases(rng, n)
    s1, s2, s6 = r(120), r(120), r(120)
    half = r(25)
    pal = half + revcomp(half)
    c0 = r(211) + s1 + r(90) + s2 + r(75) + s6 + r(33) + s6 + r(140) + pal + r(101) + s6 + r(57)
    c1 = r(97) + revcomp(s6) + "N" * 31 + r(60) + s2.lower() + r(44) + s6 + r(80) + s6 + r(119)
    return ["c0", "c1"], [c0, c1], dict(s1=s1, s2=s2, s6=s6, pal=pal)


def build_index(prefix, names, seqs):
    from uncalled_amd import build_index as bi
    codes, holes, n_ambs = bi.encode_contigs(seqs)
    bi.build_from_codes(str(prefix), names, [""] * len(names), [len(s) for s in seqs], codes, holes, n_ambs)


def make_tiny(directory):
    """the tiny reference, its index files (built on the CPU), its text as the index holds it, and room for the checker's window
    counts per min_len, which tiny_counts fills once"""
    names, seqs, parts = tiny_reference()
    prefix = directory / "tiny"
    build_index(prefix, names, seqs)
    return dict(names=names, seqs=seqs, parts=parts, prefix=prefix, text=mn.pac_text(prefix), counts={})


def tiny_counts(tiny, min_len):
    if min_len not in tiny["counts"]:
        tiny["counts"][min_len] = mn.window_counts(tiny["text"], tiny["seqs"], min_len)
    return tiny["counts"][min_len]


def load_index(capi, prefix, lib, fm32=True):
    """the index without the dense suffix array (the walk does not use it); fm32=False: UNC_FM32=0, the 64-bit arithmetic of the
    references of 2^32 rows and more on a small one (the library reads the variable while it loads the index)"""
    old = os.environ.get("UNC_FM32")
    if not fm32:
        os.environ["UNC_FM32"] = "0"
    try:
        return capi.Index(prefix, lib=lib, dense_sa=False)
    finally:
        if old is None:
            os.environ.pop("UNC_FM32", None)
        else:
            os.environ["UNC_FM32"] = old


def check_external(capi, index, text, contigs, min_len, min_copies, lib=None, naive_counts=None):
    """with and without the count tap, for every min_copy: the tap is the checker's substring count, the masks are equal"""
    counts = naive_counts if naive_counts is not None else mn.window_counts(text, contigs, min_len)
    flat = [x for row in counts for x in row]
    out = {}
    for min_copy in min_copies:
        want, _, iv, total = mn.mask_external(text, contigs, min_len, min_copy, counts)
        for tap in (True, False):
            with masker(capi, contigs, lib) as m:
                got = m.external(index, min_len, min_copy, counts=tap)
                if tap:
                    assert got[1].tolist() == flat, (min_len, min_copy)
                    got = got[0]
                assert got == total, (min_len, min_copy, tap, got, total)
                assert m.codes().tolist() == mn.codes_of(want), (min_len, min_copy, tap)
        out[min_copy] = (want, iv, total)
    return out


def check_grid_strides(capi, tiny, lib=None):
    """call with UNC_MASK_BLOCKS=2 in the environment: a grid of 2 workgroups = 512 lanes = 8 wavefronts.  The several-workgroups text
    (71 130 bases) then takes k_kmer_count round its loop 9 times (4446 chunks), k_mask_flag_kmer 9 times (4448), k_mask_cover 3
    times (1112 words) and k_kmer_argmax 512 times, the tiny reference takes k_fm_window_count 5 times (36 words over 8
    wavefronts) -- each with a last trip that only some lanes, or some wavefronts, make"""
    assert os.environ.get("UNC_MASK_BLOCKS") == "2"
    case = [c for c in internal_cases() if c["name"] == "several workgroups"][0]
    n = sum(len(s) for s in case["contigs"])
    assert (n + 15) // 16 > 8 * 512 and ((n + 15) // 16) % 512 and ((n + 63) // 64) > 2 * 512 and ((n + 63) // 64) % 512
    check_internal(capi, case, lib=lib)
    words = (sum(len(s) for s in tiny["seqs"]) + 63) // 64
    assert words > 4 * 8 and words % 8
    for fm32 in (True, False):
        ix = load_index(capi, tiny["prefix"], lib, fm32=fm32)
        check_external(capi, ix, tiny["text"], tiny["seqs"], 50, (1, 5), lib=lib, naive_counts=tiny_counts(tiny, 50))
        ix.close()


def junction_targets(text, seqs):
    """windows of 50 bases that occur in the index's text only across a junction: of the forward and the reverse strand, and of two
    contigs"""
    half = len(text) // 2
    strand = text[half - 25:half + 25]
    contig = text[len(seqs[0]) - 25:len(seqs[0]) + 25]
    return ["ACGT" + strand + "TT", contig]


def check_external_arguments(capi, index, lib=None):
    import pytest
    with masker(capi, ["ACGT" * 20], lib) as m:
        for min_len, min_copy in ((1, 1), (0, 1), (65536, 1), (50, 0)):
            with pytest.raises(capi.UncalledHipError, match="error -1"):
                m.external(index, min_len, min_copy)
        assert m.codes().tolist() == [0, 1, 2, 3] * 20
