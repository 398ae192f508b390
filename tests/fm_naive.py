"""A plain FM index for the tests: everything the device's FM layer answers (fm_dev.h, the kernels of k_taps.hip), derived from a
suffix array that is obtained by sorting the suffixes themselves.  numpy and Python integers only; no block layout, no sampling,
no 32-bit table -- nothing the device code could share a mistake with.  tests/test_fm_naive.py pins it against the oracle and a
committed digest of the reference's self-alignment on the bundled index.

Conventions are the BWA ones the reference works in (bwa_index.hpp:158-178): the matrix has rows 0 .. n, row 0 the empty suffix;
the BWT column leaves the sentinel's row (`primary`) out of every count; a range is a closed pair of rows."""
import numpy as np

NO_ROW = (1 << 64) - 1      # bwt_sa(0): the stored -1, read as uint64
KLEN = 5


class NaiveFM:
    def __init__(self, codes, lens=None):
        codes = np.ascontiguousarray(codes, dtype=np.uint8)
        self.codes = codes
        self.lens = [int(x) for x in (lens if lens is not None else [codes.size])]
        assert sum(self.lens) == codes.size and codes.size > 0 and int(codes.max()) < 4
        t = np.concatenate((codes, 3 - codes[::-1])).astype(np.uint8)       # forward strand ++ reverse complement
        n = self.n = int(t.size)
        self.t = t
        s = bytes(t + 1)                                                     # 1..4: the empty suffix sorts first
        self.sa_full = np.array(sorted(range(n + 1), key=lambda i: s[i:]), dtype=np.int64)
        assert self.sa_full[0] == n
        self.rank = np.empty(n + 1, dtype=np.int64)                          # row of the suffix that starts at a position
        self.rank[self.sa_full] = np.arange(n + 1)
        self.primary = int(self.rank[0])
        bwt = np.full(n + 1, 4, dtype=np.uint8)                              # 4: the sentinel (row `primary`)
        has_prev = self.sa_full > 0
        bwt[has_prev] = t[self.sa_full[has_prev] - 1]
        self.bwt = bwt
        counts = np.bincount(t, minlength=4)
        self.L2 = [0] + [int(x) for x in np.cumsum(counts)]                  # L2[c]: symbols smaller than c; L2[4] = n
        # cum[k + 1, c] = occurrences of c in rows 0 .. k
        self.cum = np.zeros((n + 2, 4), dtype=np.int64)
        for c in range(4):
            self.cum[1:, c] = np.cumsum(bwt == c)
        self.L2a = np.array(self.L2, dtype=np.int64)

    def occ(self, k, c):
        return int(self.cum[k + 1, c])       # (k = -1: none)

    def get_neighbor(self, s, e, c):
        return self.L2[c] + self.occ(s - 1, c) + 1, self.L2[c] + self.occ(e, c)

    def get_neighbors(self, s, e, c):
        """the same for arrays of queries -> (starts, ends) as uint64, the BWA-format pair whether or not any row is left"""
        s, e, c = np.asarray(s, dtype=np.int64), np.asarray(e, dtype=np.int64), np.asarray(c, dtype=np.int64)
        return ((self.L2a[c] + self.cum[s, c] + 1).astype(np.uint64), (self.L2a[c] + self.cum[e + 1, c]).astype(np.uint64))

    def sa(self, row):
        return NO_ROW if row == 0 else int(self.sa_full[row])

    def sa_rows(self):
        """rows 0 .. n as uint64"""
        out = self.sa_full.astype(np.uint64)
        out[0] = NO_ROW
        return out

    def kmer_ranges(self):
        """The range of every 5-mer as BwaIndex::load_index chains it: the head base's L2 pair -- which starts one row low -- then one
        backward step per further base.  Each result is tied to the suffix array itself: its rows are exactly the suffixes that start
        with the four bases stepped over, in the order of the steps reversed, and go on with a suffix of the head's (one-low) range."""
        n, L2 = self.n, self.L2
        members = [[] for _ in range(4 ** KLEN)]
        for p in range(n - KLEN + 2):                 # a start with KLEN - 1 symbols behind it; what follows may be the empty suffix
            b4, b3, b2, b1 = (int(x) for x in self.t[p:p + KLEN - 1])
            tail = int(self.rank[p + KLEN - 1])
            for h in range(4):
                if L2[h] <= tail <= L2[h + 1]:
                    members[(h << 8) | (b1 << 6) | (b2 << 4) | (b3 << 2) | b4].append(int(self.rank[p]))
        out = np.empty((4 ** KLEN, 2), dtype=np.uint64)
        for k in range(4 ** KLEN):
            h = (k >> (2 * KLEN - 2)) & 3
            s, e = L2[h], L2[h + 1]
            for i in range(1, KLEN):
                s, e = self.get_neighbor(s, e, (k >> (2 * (KLEN - i - 1))) & 3)
            assert s >= 1 and e + 1 >= s
            assert sorted(members[k]) == list(range(s, e + 1)), (k, s, e, members[k])
            # ... which is the run of suffixes that start with the whole k-mer, and at most the one row below it
            pat = bytes([((k >> (2 * j)) & 3) for j in range(KLEN)])
            whole = [r for r in range(s, e + 1) if bytes(self.t[self.sa_full[r]:self.sa_full[r] + KLEN]) == pat]
            assert whole == list(range(e + 1 - len(whole), e + 1)) and e - s + 1 - len(whole) <= 1, (k, s, e)
            out[k] = (s, e)
        return out

    def self_align(self):
        """self_align(prefix, sample_dist = 1) of the reference: from every base of every contig, the sizes of the ranges met while the
        complemented forward strand is stepped through the index, until one row is left or the contig ends -> a list of lists."""
        out, st = [], 0
        for ln in self.lens:
            for i in range(ln):
                b = 3 - int(self.codes[st + i])
                s, e = self.L2[b], self.L2[b + 1]
                sizes = []
                j = i + 1
                while j < ln and e - s + 1 > 1:
                    sizes.append(e - s + 1)
                    s, e = self.get_neighbor(s, e, 3 - int(self.codes[st + j]))
                    j += 1
                if e - s + 1 > 0:
                    sizes.append(e - s + 1)
                out.append(sizes)
            st += ln
        return out


def build(prefix, codes, lens=None):
    """the five BWA files + .uncl of a reference, written by the numpy builder -> its NaiveFM"""
    from uncalled_amd.build_index import build_from_codes
    codes = np.ascontiguousarray(codes, dtype=np.uint8)
    lens = [int(x) for x in (lens if lens is not None else [codes.size])]
    names = ["c%d" % i for i in range(len(lens))]
    info = build_from_codes(prefix, names, [""] * len(lens), lens, codes)
    fm = NaiveFM(codes, lens)
    assert info["seq_len"] == fm.n and info["primary"] == fm.primary
    return fm
