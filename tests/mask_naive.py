"""A plain checker for repeat masking (include/uncalled_hip.h: unc_mask_*): strings, dictionaries and str.find -- no numpy tricks,
no rolling codes, no bitmaps, no FM index: nothing the device code could share a mistake with.  mask_seq is written from the stated
behaviour of the reference's masking/mask_kmers.py and pinned on that script's output by tests/golden/mask_goldens.npz (tests/test_mask_cpu.py); the window
counts are substring counts over the text unpacked from <prefix>.pac followed by its reverse complement, cross-checked against
tests/fm_naive.py's interval sizes.

A reference is a list of contigs, each a string.  A base is one of ACGT in either case; every other character is "not a base"."""

BASES = "ACGT"
COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}


def kmer_code(kmer):
    code = 0
    for ch in kmer:
        code = code * 4 + BASES.index(ch)
    return code


def codes_of(contigs):
    """one code per base, as the device holds them: 0..3, and 4 for everything else"""
    out = []
    for s in contigs:
        for ch in s.upper():
            out.append(BASES.index(ch) if ch in BASES else 4)
    return out


def kmer_counts(contigs, k):
    """jellyfish count -m k without -C: every window of k bases of every contig, forward strand, overlapping ones included"""
    counts = {}
    for s in contigs:
        u = s.upper()
        for i in range(len(u) - k + 1):
            w = u[i:i + k]
            if all(ch in BASES for ch in w):
                counts[w] = counts.get(w, 0) + 1
    return counts


def top_kmer(counts):
    """the largest count; among equals the k-mer with the smallest code (ACGT order, first base most significant) -> (kmer, count)"""
    best = None
    for kmer, c in counts.items():
        if best is None or c > best[1] or (c == best[1] and kmer_code(kmer) < kmer_code(best[0])):
            best = (kmer, c)
    return best


def occurrence_starts(seq, kmer):
    """every position at which the k-mer occurs in the sequence, upper-cased; overlapping occurrences included"""
    upper, starts = seq.upper(), []
    at = upper.find(kmer)
    while at != -1:
        starts.append(at)
        at = upper.find(kmer, at + 1)
    return starts


def mask_seq(seq, kmer):
    """what masking/mask_kmers.py does to one sequence, from its stated behaviour: every character covered by an occurrence of the
    k-mer becomes N, every other one stays as it is -> (masked sequence, occurrences)"""
    starts = occurrence_starts(seq, kmer)
    covered = [False] * len(seq)
    for st in starts:
        for p in range(st, st + len(kmer)):
            covered[p] = True
    return "".join("N" if cv else ch for ch, cv in zip(seq, covered)), len(starts)


def fasta_records(text):
    """[(header line, sequence)] of a FASTA file's text; a record without sequence lines has the empty sequence"""
    records = []
    for block in text.split(">")[1:]:
        lines = block.split("\n")
        records.append((">" + lines[0].strip(), "".join(x.strip() for x in lines[1:])))
    return records


def mask_fasta_text(text, kmer):
    """the script run on a FASTA file -> (what it prints: per record the header line and the masked sequence on one line; the count
    of its line on stderr)"""
    out, total = [], 0
    for header, seq in fasta_records(text):
        masked, n = mask_seq(seq, kmer)
        out.append(header + "\n" + masked + "\n")
        total += n
    return "".join(out), total


def newly_masked(before, after):
    return sum(1 for a, b in zip("".join(before), "".join(after)) if a != b)


def mask_internal(contigs, k, iters):
    """mask_internal.sh:46-54 with the two stated departures: ties to the smallest code, and the loop ends before masking when the
    largest count is below 2 -> (masked contigs, [(kmer, occurrences, bases newly masked)] per iteration done)"""
    contigs = list(contigs)
    report = []
    for _ in range(iters):
        best = top_kmer(kmer_counts(contigs, k))
        if best is None or best[1] < 2:
            break
        kmer = best[0]
        done = [mask_seq(s, kmer) for s in contigs]
        after = [m for m, _ in done]
        report.append((kmer, sum(n for _, n in done), newly_masked(contigs, after)))
        contigs = after
    return contigs, report


def pac_text(prefix):
    """the index's text as BWA stores it: the bases of <prefix>.pac, then their reverse complement"""
    with open(str(prefix) + ".pac", "rb") as f:
        raw = f.read()
    l_pac = (len(raw) - 2) * 4 + raw[-1]
    fwd = "".join(BASES[(raw[i >> 2] >> ((3 - (i & 3)) * 2)) & 3] for i in range(l_pac))
    return fwd + "".join(COMP[ch] for ch in reversed(fwd))


def count_occurrences(text, w):
    n = 0
    i = text.find(w)
    while i >= 0:
        n += 1
        i = text.find(w, i + 1)
    return n


def window_counts(text, contigs, min_len):
    """per contig, per position: the occurrences in `text` of the window of min_len bases that starts there; 0 where there is no
    window (too close to the contig's end, or a character that is not a base inside)"""
    seen = {}
    out = []
    for s in contigs:
        u = s.upper()
        row = [0] * len(u)
        for i in range(len(u) - min_len + 1):
            w = u[i:i + min_len]
            if all(ch in BASES for ch in w):
                if w not in seen:
                    seen[w] = count_occurrences(text, w)
                row[i] = seen[w]
        out.append(row)
    return out


def mask_external(text, contigs, min_len, min_copy, counts=None):
    """mask_external.sh:61-80 -> (masked contigs, the window counts, [(contig index, start, end)] merged, bases newly masked);
    counts: what window_counts gave for the same text, contigs and min_len before (they do not depend on min_copy)"""
    if counts is None:
        counts = window_counts(text, contigs, min_len)
    masked, intervals, total = [], [], 0
    for ci, (s, row) in enumerate(zip(contigs, counts)):
        cover = [False] * len(s)
        for i, c in enumerate(row):
            if c > min_copy:
                for j in range(i, i + min_len):
                    cover[j] = True
        out = "".join("N" if cv else ch for ch, cv in zip(s, cover))
        masked.append(out)
        i = 0
        while i < len(s):
            if cover[i]:
                j = i
                while j < len(s) and cover[j]:
                    j += 1
                intervals.append((ci, i, j))
                i = j
            else:
                i += 1
        total += sum(1 for a, b in zip(s, out) if a != b)
    return masked, counts, intervals, total
