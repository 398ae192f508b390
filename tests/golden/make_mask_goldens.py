"""tests/golden/mask_goldens.npz: what the reference's own masking/mask_kmers.py prints for a handful of tiny FASTA files, run as
shipped (`python <reference>/masking/mask_kmers.py in.fa -k KMER`; it imports matplotlib, which must be installed).  For every
case: the FASTA text, the k-mer, the script's stdout and the count of its stderr line "masked %d occurences of KMER".
tests/test_mask_cpu.py pins tests/mask_naive.py on these, and the device is pinned on mask_naive.

Usage: python tests/golden/make_mask_goldens.py <checkout of the reference>

(No case has an empty record before the last one: mask_kmers.py:65 skips a record without sequence lines and its headers then
pair up with the wrong sequences.)"""
import re
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np

OUT = Path(__file__).resolve().parent / "mask_goldens.npz"

CASES = [
    ("poly-A", ">a\n" + "A" * 40 + "\n", "AAA"),
    ("stride 2", ">ac twenty times\n" + "AC" * 20 + "\n", "ACAC"),
    ("adjacent to itself", ">adj\nACGTACGTTTGCA\n", "ACGT"),
    ("records, lines, case, N", ">one first\nACG\n>two\nAC\n>three\nTTGA\nCG\n>four\nTTAC\n>five\nGTT\n>six x y\nNNacgNN\nACGnAC\nGN\n>seven\nacN\n", "ACG"),
    ("overlap across lines", ">r\nTTAAA\nAAT\nAAAC\n", "AAA"),
    ("absent", ">r\nACGTACGT\n>s\nGGGG\n", "TTT"),
    ("whole record", ">r\nGATTACA\n>s\nGATTACAGATTACA\n", "GATTACA"),
]


def main():
    script = Path(sys.argv[1]) / "masking" / "mask_kmers.py"
    names, fastas, kmers, outs, counts = [], [], [], [], []
    with tempfile.TemporaryDirectory() as tmp:
        for name, fasta, kmer in CASES:
            fa = Path(tmp) / "in.fa"
            fa.write_text(fasta)
            r = subprocess.run([sys.executable, str(script), str(fa), "-k", kmer], capture_output=True, text=True, check=True)
            m = re.fullmatch(r"masked (\d+) occurences of %s\n" % kmer, r.stderr)
            assert m, r.stderr
            names.append(name); fastas.append(fasta); kmers.append(kmer); outs.append(r.stdout); counts.append(int(m.group(1)))
    np.savez(OUT, name=np.array(names), fasta=np.array(fastas), kmer=np.array(kmers), stdout=np.array(outs),
             count=np.array(counts, dtype=np.int64))
    print("wrote", OUT, counts)


if __name__ == "__main__":
    main()
