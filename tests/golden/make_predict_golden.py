#!/usr/bin/env python3
"""Capture tests/golden/predict_clusters.json from the REFERENCE's own cluster_basedon_location
(utils/cluster_basedon_location.py): seeded coordinate-sorted SAM inputs and the cluster table it writes for each.

    python tests/golden/make_predict_golden.py <reference src/mirge directory>

Run only in the build container: the one module is copied to a scratch directory outside the
repository, CRLF stripped, converted with lib2to3 where the interpreter still has it, and imported from there.  Only
data is written into the repository: per input the file name, the SAM text and the TSV text of every threshold.

Cases: thresholds 1, 8, 14 and 15 over random worlds (both strands interleaved, names with and without "chr", FLAG 4
rows, reads of 16-40 nt whose tails past the 25-nt seed disagree with their neighbours, equal starts of different
lengths) and hand-made shapes (nested alignments, chains, an alignment shorter than the threshold inside a longer one,
one empty file, one file with only unaligned reads).
"""
import importlib.util
import json
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "predict_clusters.json")
ENTRIES = ["chr1", "scaffold_12", "chr2_random", "chrX", "KI270728.1"]


def load_reference(src):
    tmp = tempfile.mkdtemp(prefix="predict_golden_")
    dst = os.path.join(tmp, "cluster_basedon_location.py")
    shutil.copy(os.path.join(src, "utils", "cluster_basedon_location.py"), dst)
    os.chmod(dst, 0o644)
    with open(dst, "rb") as fh:
        data = fh.read().replace(b"\r\n", b"\n")
    with open(dst, "wb") as fh:
        fh.write(data)
    subprocess.run([sys.executable, "-m", "lib2to3", "-w", "-n", dst], capture_output=True)   # (absent in new Pythons)
    spec = importlib.util.spec_from_file_location("cluster_basedon_location", dst)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return tmp, mod.cluster_basedon_location


def rnd(rng, n):
    return "".join("ACGT"[c] for c in rng.integers(0, 4, n))


def sam_line(name, flag, chrom, pos, seq):
    if flag == 4:
        return "%s\t4\t*\t0\t0\t*\t*\t0\t0\t%s\t%s\tXM:i:0\n" % (name, seq, "I" * len(seq))
    return "%s\t%d\t%s\t%d\t255\t%dM\t*\t0\t0\t%s\t%s\tXA:i:0\tMD:Z:%d\tNM:i:0\n" % (
        name, flag, chrom, pos, len(seq), seq, "I" * len(seq), len(seq))


def header():
    return "@HD\tVN:1.0\tSO:coordinate\n" + "".join("@SQ\tSN:%s\tLN:5000\n" % e for e in ENTRIES)


def assemble(rows, unaligned):
    """rows: (entry index, pos, strand, seq) in any order -> SAM text in coordinate order, names mir<k>_<count>."""
    rows = sorted(enumerate(rows), key=lambda x: (x[1][0], x[1][1], x[1][2], x[0]))
    out, k = [header()], 0
    for _, (e, pos, strand, seq) in rows:
        out.append(sam_line("mir%d_%d" % (k, 1 + (k * 7) % 23), 16 if strand else 0, ENTRIES[e], pos, seq))
        k += 1
    for seq in unaligned:
        out.append(sam_line("mir%d_%d" % (k, 2), 4, "*", 0, seq))
        k += 1
    return "".join(out)


def random_world(seed):
    rng = np.random.default_rng(seed)
    genome = [rnd(rng, 1200) for _ in ENTRIES]
    rows = []
    for _ in range(int(rng.integers(40, 90))):
        e = int(rng.integers(0, len(ENTRIES)))
        # piles: starts drawn around a few loci, so that overlaps of every size occur
        locus = int(rng.choice([100, 130, 400, 415, 800]))
        pos = max(1, locus + int(rng.integers(-30, 31)))
        L = int(rng.integers(16, 41))
        seq = genome[e][pos - 1:pos - 1 + L]
        if L > 25 and rng.random() < 0.6:          # mismatches past the seed: tails that disagree with the neighbours
            i = int(rng.integers(25, L))
            seq = seq[:i] + "ACGT"[("ACGT".index(seq[i]) + 1) % 4] + seq[i + 1:]
        if rng.random() < 0.05:
            i = int(rng.integers(0, L))
            seq = seq[:i] + "N" + seq[i + 1:]
        rows.append((e, pos, int(rng.integers(0, 2)), seq))
        if rng.random() < 0.15:                    # an equal start of another length
            rows.append((e, pos, rows[-1][2], genome[e][pos - 1:pos - 1 + int(rng.integers(16, 41))]))
    return assemble(rows, [rnd(rng, int(rng.integers(16, 30))) for _ in range(int(rng.integers(0, 5)))])


def shapes():
    rng = np.random.default_rng(99)
    g = rnd(rng, 400)
    cut = lambda pos, L: g[pos - 1:pos - 1 + L]
    nested = [(0, 10, 0, cut(10, 40)), (0, 12, 0, cut(12, 20)), (0, 15, 0, cut(15, 16)), (0, 30, 0, cut(30, 25)),
              (0, 10, 1, cut(10, 40)), (0, 20, 1, cut(20, 18))]
    chain = [(3, 100 + 8 * i, i % 2, cut(100 + 8 * i, 22)) for i in range(12)] + \
            [(3, 100 + 8 * i, 0, cut(100 + 8 * i, 22)) for i in range(1, 12, 2)]
    # a short alignment inside a long one, ending before it: the next one meets the long one's end
    inside = [(0, 50, 0, cut(50, 40)), (0, 78, 0, cut(78, 16)), (0, 80, 0, cut(80, 16)), (0, 82, 0, cut(82, 30)),
              (0, 120, 0, cut(120, 16)), (0, 121, 0, cut(121, 16))]
    equal = [(2, 60, 0, cut(60, 16)), (2, 60, 0, cut(60, 30)), (2, 60, 0, cut(60, 22)), (2, 60, 1, cut(60, 35)),
             (2, 60, 1, cut(60, 17)), (1, 60, 0, cut(60, 30)), (4, 60, 0, cut(60, 30))]
    return [("nested", assemble(nested, [])), ("chain", assemble(chain, [cut(1, 20)])), ("inside", assemble(inside, [])),
            ("equal", assemble(equal, [])), ("empty", ""), ("header_only", header()),
            ("unaligned_only", assemble([], [cut(5, 20), cut(9, 18)]))]


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    tmp, reference = load_reference(sys.argv[1])
    inputs = [("world%d" % s, random_world(s)) for s in range(8)] + shapes()
    cases = []
    try:
        for name, sam in inputs:
            fname = "mapped_mirna_%s_vs_genome_sorted.sam" % name
            path = os.path.join(tmp, fname)
            with open(path, "w") as fh:
                fh.write(sam)
            tsv = {}
            for t in (1, 8, 14, 15):
                reference(path, str(t))
                with open(path[:-4] + "_clusters.tsv") as fh:
                    tsv[str(t)] = fh.read()
            cases.append(dict(file=fname, sam=sam, tsv=tsv))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    with open(OUT, "w") as fh:
        json.dump(dict(source="reference utils/cluster_basedon_location.py", cases=cases), fh, indent=0)
    print("wrote %s: %d inputs, %d bytes" % (OUT, len(cases), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
