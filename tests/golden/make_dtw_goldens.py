#!/usr/bin/env python3
"""Generates tests/golden/dtw_goldens.npz: what the reference's DTW<float, u16, Func> (src/dtw.hpp), its two cost functions and
seq_to_kmers / kmers_revcomp (src/bp.hpp) give on small inputs.  Container-only (needs the reference's sources): a small harness
of our own is written into a temporary directory, includes the reference's headers WHERE THEY LIE, is compiled with the
reference's flags (oracle/Makefile CXXFLAGS_REF) and dumps results; nothing of the reference enters the tree, only its outputs.

  python tests/golden/make_dtw_goldens.py [--time ROWS COLS]     (--time: the reference's single-thread cells/s on this host)
"""
import os
import struct
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
G = Path(__file__).resolve().parent
REF = Path(os.environ.get("REF", "/root/reference"))      # as oracle/Makefile
PAC = G / "example_index" / "example_ref.pac"

HARNESS = r"""
#include <iostream>
#include <math.h>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <vector>
#include "model_r94.inl"
#include "pore_model.hpp"
#include "bp.hpp"
#include "dtw.hpp"

template <class T> static T rd(FILE *f) { T v; if (fread(&v, sizeof v, 1, f) != 1) { fprintf(stderr, "short input\n"); exit(2); } return v; }
template <class T> static void wr(FILE *f, T v) { fwrite(&v, sizeof v, 1, f); }

template <class D> static void run(FILE *out, const std::vector<float> &ev, const std::vector<u16> &km, const DTWParams &p) {
    D d(ev, km, p);
    wr<float>(out, d.score());
    wr<float>(out, d.mean_score());
    auto path = d.get_path();
    wr<u64>(out, path.size());
    for (auto &q : path) { wr<u32>(out, (u32)q.first); wr<u32>(out, (u32)q.second); }
}

int main(int argc, char **argv) {
    std::string mode = argv[1];
    if (mode == "time") {
        u32 rows = atoi(argv[2]), cols = atoi(argv[3]);
        std::vector<float> ev(cols); std::vector<u16> km(rows);
        for (u32 i = 0; i < cols; i++) ev[i] = 70.f + (float)((i * 2654435761u) >> 20) * 0.01f;
        for (u32 i = 0; i < rows; i++) km[i] = (u16)((i * 40503u) & 1023);
        for (int cost = 0; cost < 2; cost++) {
            auto t0 = std::chrono::steady_clock::now();
            float s;
            if (cost == 0) { DTWr94p d(ev, km, DTW_EVENT_GLOB); s = d.score(); } else { DTWr94d d(ev, km, DTW_EVENT_GLOB); s = d.score(); }
            double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            printf("%s %u x %u: %.3f s, %.3e cells/s (score %g)\n", cost ? "r94d" : "r94p", rows, cols, sec, (double)rows * cols / sec, s);
        }
        return 0;
    }
    FILE *in = fopen(argv[2], "rb"), *out = fopen(argv[3], "wb");
    if (mode == "dtw") {
        u32 n = rd<u32>(in);
        for (u32 c = 0; c < n; c++) {
            u32 subseq = rd<u32>(in), cost = rd<u32>(in);
            DTWParams p;
            p.subseq = subseq == 0 ? DTWSubSeq::NONE : subseq == 1 ? DTWSubSeq::ROW : DTWSubSeq::COL;
            p.dw = rd<float>(in); p.hw = rd<float>(in); p.vw = rd<float>(in);
            u32 cols = rd<u32>(in), rows = rd<u32>(in);
            std::vector<float> ev(cols); std::vector<u16> km(rows);
            for (auto &e : ev) e = rd<float>(in);
            for (auto &k : km) k = rd<u16>(in);
            if (cost == 0) run<DTWr94p>(out, ev, km, p); else run<DTWr94d>(out, ev, km, p);
        }
    } else if (mode == "cost") {
        for (u32 k = 0; k < 1024; k++) wr<float>(out, pmodel_r94_template.get_mean((u16)k));
        u32 n = rd<u32>(in);
        for (u32 i = 0; i < n; i++) {
            u16 k = rd<u16>(in); float e = rd<float>(in);
            wr<float>(out, dtwcost_r94p(k, e)); wr<float>(out, dtwcost_r94d(k, e));
        }
    } else if (mode == "kmers") {
        FILE *pf = fopen(argv[4], "rb");
        std::vector<u8> pac;
        int ch;
        while ((ch = fgetc(pf)) != EOF) pac.push_back((u8)ch);
        pac.resize(pac.size() + 8);
        u32 n = rd<u32>(in);
        for (u32 i = 0; i < n; i++) {
            u64 st = rd<u64>(in), en = rd<u64>(in);
            auto f = seq_to_kmers<KmerLen::k5>(pac.data(), st, en);
            auto r = kmers_revcomp<KmerLen::k5>(f);
            wr<u64>(out, f.size());
            for (u16 k : f) wr<u16>(out, k);
            for (u16 k : r) wr<u16>(out, k);
        }
    }
    fclose(out);
    return 0;
}
"""

SUBSEQS = (0, 1, 2)                                  # NONE, ROW, COL
COSTS = (0, 1)                                       # r94p, r94d
WEIGHTS = ((2, 1, 100), (10, 1, 1000), (1, 1, 1))
SHAPES = ((1, 1), (1, 9), (9, 1), (1, 70), (70, 1), (5, 5), (17, 33), (64, 64), (65, 63), (128, 40), (40, 130), (129, 200),
          (300, 300), (300, 90), (100, 290), (63, 65), (2, 2), (200, 129))        # (rows = k-mers, cols = events)


def build_harness(tmp):
    src = Path(tmp) / "dtw_harness.cpp"
    src.write_text(HARNESS)
    exe = Path(tmp) / "dtw_harness"
    subprocess.run(["g++", "-std=c++11", "-O3", "-fPIC", "-w", "-I", str(ROOT / "oracle" / "shim"), "-I", str(REF / "src"),
                    str(src), "-o", str(exe)], check=True)
    return exe


def walk_kmers(rng, n, repeat_runs=False):
    """k-mers of a random base sequence (consecutive k-mers overlap by four bases); repeat_runs: homopolymer stretches, whose
    k-mers repeat"""
    bases = rng.integers(0, 4, n + 4)
    if repeat_runs:
        for st in range(3, n, 23):
            bases[st:st + 11] = bases[st]
    k = np.zeros(n, np.uint16)
    for i in range(n):
        v = 0
        for b in bases[i:i + 5]:
            v = (v << 2) | int(b)
        k[i] = v
    return k


def events_for(rng, kmers, cols, means, noise):
    """`cols` event means that follow the k-mers' model means with stays and skips"""
    pos = np.sort(rng.integers(0, kmers.size, cols))
    return (means[kmers[pos]] + noise * rng.standard_normal(cols)).astype(np.float32)


def main():
    from dtw_check import Checker
    from uncalled_amd import capi
    if len(sys.argv) > 1 and sys.argv[1] == "--time":
        with tempfile.TemporaryDirectory() as tmp:
            exe = build_harness(tmp)
            print(subprocess.run([str(exe), "time", sys.argv[2], sys.argv[3]], check=True, capture_output=True, text=True).stdout)
        return
    rng = np.random.default_rng(20261017)
    with tempfile.TemporaryDirectory() as tmp:
        tmp = Path(tmp)
        exe = build_harness(tmp)
        # ---- cost functions and the template model's means
        ck = rng.integers(0, 1024, 400).astype(np.uint16)
        ce = rng.uniform(40, 140, 400).astype(np.float32)
        ours = capi.dtw_model_tables()[0]
        ce[0] = ours[ck[0]] + np.float32(0.37)       # the reference's `abs` is the float overload: this point costs 0.37, not 0
        with open(tmp / "cost.in", "wb") as f:
            f.write(struct.pack("<I", ck.size))
            for k, e in zip(ck, ce):
                f.write(struct.pack("<Hf", int(k), float(e)))
        subprocess.run([str(exe), "cost", str(tmp / "cost.in"), str(tmp / "cost.out")], check=True)
        raw = np.fromfile(tmp / "cost.out", dtype=np.float32)
        means = raw[:1024].copy()
        cost_out = raw[1024:].reshape(-1, 2)
        assert np.array_equal(means.view(np.uint32), ours.view(np.uint32)), "template means differ from the library's"
        assert 0.3 < cost_out[0, 1] < 0.45, cost_out[0]
        # ---- alignments
        cases = []
        combos = [(s, c, w) for s in SUBSEQS for c in COSTS for w in WEIGHTS]
        for ci, (s, c, w) in enumerate(combos):
            for si in range(6):
                rows, cols = SHAPES[(ci * 5 + si * 3) % len(SHAPES)] if si else SHAPES[ci % len(SHAPES)]
                km = walk_kmers(rng, rows)
                ev = events_for(rng, km, cols, means, 1.5) if si % 2 == 0 else rng.uniform(60, 130, cols).astype(np.float32)
                cases.append(dict(subseq=s, cost=c, w=w, ev=ev, km=km, tie=0))
        for s in SUBSEQS:      # tie-heavy: events exactly on the model means, without and with runs of repeated k-mers (r94d: cost 0 on the path)
            for w in WEIGHTS:
                km = walk_kmers(rng, 90)
                cases.append(dict(subseq=s, cost=1, w=w, ev=means[km[np.sort(np.concatenate([np.arange(90), rng.integers(0, 90, 30)]))]].astype(np.float32), km=km, tie=1))
                km = walk_kmers(rng, 150, repeat_runs=True)
                ev = means[km[np.sort(np.concatenate([np.arange(150), rng.integers(0, 150, 20)]))]].astype(np.float32)
                cases.append(dict(subseq=s, cost=1, w=w, ev=ev, km=km, tie=1))
        with open(tmp / "dtw.in", "wb") as f:
            f.write(struct.pack("<I", len(cases)))
            for c in cases:
                f.write(struct.pack("<IIfffII", c["subseq"], c["cost"], *map(float, c["w"]), c["ev"].size, c["km"].size))
                f.write(c["ev"].astype("<f4").tobytes())
                f.write(c["km"].astype("<u2").tobytes())
        subprocess.run([str(exe), "dtw", str(tmp / "dtw.in"), str(tmp / "dtw.out")], check=True)
        blob = (tmp / "dtw.out").read_bytes()
        at = 0
        chk = Checker()
        n_tie_cells = []
        for c in cases:
            c["score"], c["mean"], n = struct.unpack_from("<IIQ", blob, at)
            at += 16
            c["path"] = np.frombuffer(blob, dtype="<u4", count=2 * n, offset=at).reshape(n, 2).copy()
            at += 8 * n
            # our checker must agree bit for bit, and must see ties where ties are wanted
            r = chk.dtw(c["ev"], c["km"], c["subseq"], c["cost"], *c["w"])
            assert r["score_bits"] == c["score"] and np.array_equal(r["path"], c["path"]), "the checker disagrees with the reference"
            n_tie_cells.append(r["ties"])
            if c["tie"]:
                assert r["ties"] >= 1, "a tie case without ties"
        assert at == len(blob)
        # ---- seq_to_kmers / kmers_revcomp on the example reference: all four values of st & 3 and en & 3
        l_pac = (PAC.stat().st_size - 1) * 4 - 4      # (a lower bound of the packed length: the file ends in a count byte)
        ranges = [(st, st + ln) for st, ln in ((0, 40), (1, 43), (2, 40), (3, 41), (1000, 5), (1001, 6), (4098, 131), (2003, 64),
                                               (3002, 9), (5001, 258), (7000, 4), (8003, 1022), (1234, 600), (7, 300), (9000, 1000))]
        assert {st & 3 for st, _ in ranges} == {0, 1, 2, 3} and {en & 3 for _, en in ranges} == {0, 1, 2, 3}
        assert max(en for _, en in ranges) <= l_pac
        with open(tmp / "km.in", "wb") as f:
            f.write(struct.pack("<I", len(ranges)))
            for st, en in ranges:
                f.write(struct.pack("<QQ", st, en))
        subprocess.run([str(exe), "kmers", str(tmp / "km.in"), str(tmp / "km.out"), str(PAC)], check=True)
        blob = (tmp / "km.out").read_bytes()
        at, kf, kr, koff = 0, [], [], [0]
        for _ in ranges:
            (n,) = struct.unpack_from("<Q", blob, at)
            at += 8
            kf.append(np.frombuffer(blob, dtype="<u2", count=n, offset=at)); at += 2 * n
            kr.append(np.frombuffer(blob, dtype="<u2", count=n, offset=at)); at += 2 * n
            koff.append(koff[-1] + n)
    ev_off = np.cumsum([0] + [c["ev"].size for c in cases]).astype(np.uint64)
    km_off = np.cumsum([0] + [c["km"].size for c in cases]).astype(np.uint64)
    path_off = np.cumsum([0] + [c["path"].shape[0] for c in cases]).astype(np.uint64)
    out = G / "dtw_goldens.npz"
    np.savez_compressed(
        out,
        subseq=np.array([c["subseq"] for c in cases], np.uint32), cost=np.array([c["cost"] for c in cases], np.uint32),
        weights=np.array([c["w"] for c in cases], np.float32), tie_case=np.array([c["tie"] for c in cases], np.uint8),
        tie_cells=np.array(n_tie_cells, np.uint32),
        events=np.concatenate([c["ev"] for c in cases]), ev_off=ev_off,
        kmers=np.concatenate([c["km"] for c in cases]), km_off=km_off,
        score_bits=np.array([c["score"] for c in cases], np.uint32), mean_bits=np.array([c["mean"] for c in cases], np.uint32),
        path=np.concatenate([c["path"] for c in cases]).astype(np.uint16), path_off=path_off,
        cost_kmer=ck, cost_event=ce, cost_r94p_bits=cost_out[:, 0].copy().view(np.uint32), cost_r94d_bits=cost_out[:, 1].copy().view(np.uint32),
        model_mean_bits=means.view(np.uint32),
        kmer_ranges=np.array(ranges, np.uint64), kmers_fwd=np.concatenate(kf), kmers_rev=np.concatenate(kr),
        kmers_off=np.array(koff, np.uint64))
    print("wrote", out, out.stat().st_size, "bytes;", len(cases), "alignments,", sum(c["tie"] for c in cases), "tie-heavy, tie cells",
          [n_tie_cells[i] for i, c in enumerate(cases) if c["tie"]])


if __name__ == "__main__":
    main()
