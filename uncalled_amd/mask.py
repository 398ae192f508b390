"""Repeat masking of a FASTA reference on the GPU: the two recipes of the reference's masking/ directory (mask_internal.sh with
mask_kmers.py, and mask_external.sh), without jellyfish, bowtie, bedtools or samtools.  The semantics -- and the two places where
they leave the scripts: ties go to the smallest k-mer, and the loop ends when no k-mer is left that occurs twice -- are written
down in include/uncalled_hip.h (unc_mask_*) and DESIGN.md; the work is done by capi.Masker."""
import numpy as np

from . import build_index, capi


def kmer_str(code, k):
    return "".join("ACGT"[(int(code) >> (2 * (k - 1 - i))) & 3] for i in range(k))


def encode(seqs):
    """sequences -> (one code per base: 0..3 for ACGT in either case, 4 for everything else; the contigs' offsets, len(seqs) + 1)"""
    parts = [build_index._CODE[np.frombuffer(s.encode(), dtype=np.uint8)] for s in seqs]
    codes = np.concatenate(parts) if parts else np.zeros(0, np.uint8)
    return codes, np.cumsum([0] + [len(s) for s in seqs]).astype(np.uint64)


def apply_mask(seqs, before, after):
    """the sequences with N wherever a base was masked; every other character as it was (case and IUPAC letters kept)"""
    out, st = [], 0
    for s in seqs:
        raw = np.frombuffer(s.encode(), dtype=np.uint8).copy()
        raw[(after[st:st + len(s)] == 4) & (before[st:st + len(s)] != 4)] = ord("N")
        out.append(raw.tobytes().decode())
        st += len(s)
    return out


def masked_intervals(names, lens, before, after):
    """[(contig, start, end)]: the merged runs of newly masked bases, contig by contig (mask_external.sh:77-78)"""
    out, st = [], 0
    for name, ln in zip(names, lens):
        hit = np.concatenate(([0], ((after[st:st + ln] == 4) & (before[st:st + ln] != 4)).astype(np.int8), [0]))
        edges = np.flatnonzero(np.diff(hit))
        out += [(name, int(a), int(b)) for a, b in zip(edges[::2], edges[1::2])]
        st += ln
    return out


def headers(names, annos):
    return [">" + n + (" " + a if a else "") for n, a in zip(names, annos)]


def mask_internal(fasta, k, iters, device=0, lib=None):
    """mask_internal.sh <fasta> <k> <iters>: -> dict(headers, seqs (masked), report = [(k-mer, occurrences, bases masked)] per
    iteration done)"""
    names, annos, seqs = build_index.read_fasta(fasta)
    before, off = encode(seqs)
    with capi.Masker(before, off, device=device, lib=lib) as m:
        report = [(kmer_str(code, k), occ, bases) for code, occ, bases in m.internal(k, iters)]
        after = m.codes()
    return dict(headers=headers(names, annos), seqs=apply_mask(seqs, before, after), report=report)


def mask_external(index_prefix, target_fasta, min_len, min_copy, device=0, lib=None):
    """mask_external.sh <index> <target> <min_len> <min_copy>: -> dict(headers, seqs (masked), intervals = [(contig, start, end)],
    masked_bp)"""
    names, annos, seqs = build_index.read_fasta(target_fasta)
    before, off = encode(seqs)
    # the look-ups walk the BWT only: the index is loaded without the dense suffix array (six bytes a row)
    index = capi.Index(index_prefix, device=device, lib=lib, dense_sa=False)
    try:
        with capi.Masker(before, off, device=device, lib=lib) as m:
            masked_bp = m.external(index, min_len, min_copy)
            after = m.codes()
    finally:
        index.close()
    iv = masked_intervals(names, [len(s) for s in seqs], before, after)
    assert sum(b - a for _, a, b in iv) == masked_bp
    return dict(headers=headers(names, annos), seqs=apply_mask(seqs, before, after), intervals=iv, masked_bp=masked_bp)


def write_fasta(path, hdrs, seqs):
    """a record = the header line and the sequence on one line, as mask_kmers.py:80-82 prints it"""
    with open(path, "w") as f:
        for h, s in zip(hdrs, seqs):
            f.write(h + "\n" + s + "\n")


def internal_cmd(args, err, out):
    r = mask_internal(args.reference, args.k, args.iters, device=args.device)
    for i, (kmer, occ, _) in enumerate(r["report"]):
        err.write("Iteration %d: masked %d occurences of %s\n" % (i, occ, kmer))        # (mask_internal.sh:51, mask_kmers.py:78: its spelling)
    write_fasta("%smask%d.fa" % (args.out_prefix, len(r["report"])), r["headers"], r["seqs"])


def external_cmd(args, err, out):
    r = mask_external(args.index_prefix, args.target, args.min_len, args.min_copy, device=args.device)
    with open("%sreps_m%d.bed" % (args.out_prefix, args.min_copy), "w") as f:
        for name, a, b in r["intervals"]:
            f.write("%s\t%d\t%d\n" % (name, a, b))
    write_fasta("%smasked%d.fa" % (args.out_prefix, args.min_copy), r["headers"], r["seqs"])
    out.write("Masked %d basepairs\n" % r["masked_bp"])


def add_opts(p):
    sp = p.add_subparsers(dest="mask_mode")
    sp.required = True
    q = sp.add_parser("internal", help="Mask the most frequent k-mer of the reference, ITERS times over (mask_internal.sh)")
    q.add_argument("reference", type=str, help="FASTA file of the reference to mask")
    q.add_argument("k", type=int, help="k-mer length (1..13)")
    q.add_argument("iters", type=int, help="number of masking iterations to run; the run ends early once no k-mer occurs twice")
    q.add_argument("out_prefix", type=str, help="writes OUT_PREFIX + mask<iterations done>.fa")
    q.add_argument("--device", type=int, default=0, help="GPU ordinal")
    q = sp.add_parser("external", help="Mask what of the target occurs more than MIN_COPY times in an index (mask_external.sh)")
    q.add_argument("index_prefix", type=str, help="BWA prefix of the index to search for repeats of sequences in the target")
    q.add_argument("target", type=str, help="FASTA file of the target reference")
    q.add_argument("min_len", type=int, help="minimum repeat length (2..65535)")
    q.add_argument("min_copy", type=int, help="windows with more than this many exact copies in the index, both strands counted, are masked")
    q.add_argument("out_prefix", type=str, help="writes OUT_PREFIX + reps_m<min_copy>.bed and OUT_PREFIX + masked<min_copy>.fa")
    q.add_argument("--device", type=int, default=0, help="GPU ordinal")


def run(args, err=None, out=None):
    import sys
    (internal_cmd if args.mask_mode == "internal" else external_cmd)(args, err or sys.stderr, out or sys.stdout)
