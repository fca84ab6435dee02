#!/usr/bin/env python3
"""Capture tests/golden/predict_trim.json from the REFERENCE's own preTrimClusteredSeq (utils/preTrimClusteredSeq.py) and
generate_Seq (utils/generate_Seq.py): seeded cluster tables and repeat elements, and the three files it writes for each.

    python tests/golden/make_predict_trim_golden.py <reference src/mirge directory>

Run only in the build container: the two modules are copied to a scratch directory outside the repository, CRLF stripped,
converted with lib2to3, and imported from there next to a stand-in for the two Biopython names they import (Seq with
reverse_complement and __str__; generic_dna), which this script writes into that directory.  scipy's own cKDTree answers the
queries.  Only data is written into the repository: per world the cluster table's text, the elements, the cutoff and the
three output texts.

The reference's CoordinateDic comes from a pickle whose builder is not in the reference tree; here CoordinateDic[chr] =
[[cKDTree of the points (start, 0)], [(start, end, name), ...]] in one element order, which is what its query
`[(start, 0)]` and its indexing imply.

Every world but the last is generated so that no cluster's two nearest elements depend on an order among equal distances
(the model under both orders picks the same two, asserted below), so the reference alone fixes every row of those worlds.
The last world ("ties") holds equal starts and equal distances on the two sides on purpose.
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
sys.path.insert(0, os.path.dirname(HERE))
import predict_trim_model as model  # noqa: E402

OUT = os.path.join(HERE, "predict_trim.json")
TABLE_HEADER = "miRClusterID\tChr\tStrand\tStart\tEnd\tSequence\tSequenceLenght\tCoutOfReads\tCountOfMembers\tMembers\n"
BIO_SEQ = '''class Seq(object):
    def __init__(self, data, alphabet=None):
        self.data = data

    def reverse_complement(self):
        return Seq(self.data[::-1].translate(str.maketrans("ACGTacgt", "TGCAtgca")))

    def __str__(self):
        return self.data
'''


def load_reference(src):
    tmp = tempfile.mkdtemp(prefix="predict_trim_golden_")
    os.mkdir(os.path.join(tmp, "Bio"))
    for fn, text in (("__init__.py", ""), ("Seq.py", BIO_SEQ), ("Alphabet.py", "generic_dna = None\n")):
        with open(os.path.join(tmp, "Bio", fn), "w") as fh:
            fh.write(text)
    sys.path.insert(0, tmp)
    funcs = []
    for name in ("preTrimClusteredSeq", "generate_Seq"):
        dst = os.path.join(tmp, name + ".py")
        with open(os.path.join(src, "utils", name + ".py"), "rb") as fh:
            data = fh.read().replace(b"\r\n", b"\n")
        with open(dst, "wb") as fh:
            fh.write(data)
        subprocess.run([sys.executable, "-m", "lib2to3", "-w", "-n", dst], capture_output=True)
        spec = importlib.util.spec_from_file_location(name, dst)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        funcs.append(getattr(mod, name))
    return tmp, funcs[0], funcs[1]


def coordinate_dic(elements):
    from scipy.spatial import cKDTree
    return {ch: [[cKDTree([(e[0], 0) for e in els])], [tuple(e) for e in els]] for ch, els in elements.items() if els}


def rnd(rng, n, p_n=0.0):
    s = "".join("ACGT"[c] for c in rng.integers(0, 4, n))
    if n and rng.random() < p_n:
        i = int(rng.integers(0, n))
        s = s[:i] + "N" + s[i + 1:]
    return s


def table(rows, sample="smp"):
    """rows: (chr, strand, start, sequence) -> the cluster table's text (End from the length, made-up counts and members)."""
    out = [TABLE_HEADER]
    for i, (ch, strand, start, seq) in enumerate(rows):
        members = ",".join("mir%d_%d" % (7 * i + k, 2 + k) for k in range(1 + i % 3))
        out.append("%s:miRCluster_%d_%d\t%s\t%s\t%d\t%d\t%s\t%d\t%d\t%d\t%s\n" % (
            sample, i + 1, len(seq), ch, strand, start, start + len(seq) - 1, seq, len(seq), 5 + 3 * i, 1 + i % 3, members))
    return "".join(out)


def tie_free(elements, ch, start):
    rep_off, rs, _, _, _ = model.flat_repeats([ch], elements)
    return model.nearest_two(rs, 0, rep_off[1], start) == model.nearest_two(rs, 0, rep_off[1], start, high_first=True)


def random_rows(rng, elements, chroms, n, lens, span, p_minus=0.5):
    """n clusters with starts drawn near elements and far from them, redrawn until the two nearest elements are unique."""
    rows = []
    while len(rows) < n:
        ch = chroms[int(rng.integers(0, len(chroms)))]
        els = elements.get(ch, [])
        if els and rng.random() < 0.7:
            e = els[int(rng.integers(0, len(els)))]
            start = max(1, int(e[0]) + int(rng.integers(-40, 41)))
        else:
            start = int(rng.integers(1, span))
        if not tie_free(elements, ch, start):
            continue
        rows.append((ch, "-" if rng.random() < p_minus else "+", start, rnd(rng, int(rng.choice(lens)), 0.15)))
    return rows


def distinct_elements(rng, n, span, prefix, max_len=60):
    starts = rng.choice(np.arange(1, span), size=n, replace=False)
    return [[int(s), int(s) + int(rng.integers(0, max_len)), "%s%d" % (prefix, i % 7)] for i, s in enumerate(starts)]


def worlds():
    rng = np.random.default_rng(20260)
    w = []
    # chromosomes without a table: strands, N, the cutoff and one above it
    rows = [("chr1", "+", 100, rnd(rng, 30)), ("chr1", "-", 100, rnd(rng, 30)), ("chr1", "+", 200, rnd(rng, 31)),
            ("chr1", "-", 200, rnd(rng, 31)), ("chr2", "+", 5, "ACGTNACGTNACGTNACGT"), ("chr2", "-", 5, "NACGTTGCANNACGGTA"),
            ("chr2", "+", 50, "A"), ("chr2", "-", 50, "T"), ("chr2", "-", 60, "N")]
    rows += random_rows(rng, {}, ["chr1", "chr2", "chrX"], 20, [16, 22, 29, 30, 31, 40], 5000)
    w.append(("no_table", rows, {}, 30))
    # the ends of OriginalSeq: runs of 5, 6 and 7 on both strands (on `-` the run is the other letter at the other end)
    rows = []
    mid = "CGCGTACGTACG"
    for k in (5, 6, 7):
        rows += [("chr1", "+", 100 * k, mid + "A" * k), ("chr1", "+", 100 * k + 40, "T" * k + mid),
                 ("chr1", "-", 100 * k, "T" * k + mid), ("chr1", "-", 100 * k + 40, mid + "A" * k),
                 ("chr1", "+", 100 * k + 80, "A" * k + mid), ("chr1", "+", 100 * k + 90, mid + "T" * k),
                 ("chr1", "-", 100 * k + 80, mid + "T" * k), ("chr1", "-", 100 * k + 90, "A" * k + mid),
                 ("chr1", "+", 100 * k + 95, "G" + "A" * k), ("chr1", "+", 100 * k + 97, mid[:6] + "A" * k + "C")]
    rows += [("chr1", "+", 2000, "A" * 20), ("chr1", "-", 2000, "A" * 20), ("chr1", "+", 2100, "T" * 20), ("chr1", "-", 2100, "T" * 20),
             ("chr1", "+", 2200, "A" * 6), ("chr1", "-", 2200, "A" * 6), ("chr1", "+", 2300, "AAAAA"), ("chr1", "+", 2400, "TTTTT"),
             # inside an element: the end test fails first, so the name stays `*`
             ("chr3", "+", 1000, mid + "A" * 6), ("chr3", "+", 1000, mid + "A" * 5), ("chr3", "-", 1000, mid + "A" * 6),
             ("chr3", "+", 1000, rnd(rng, 31))]
    w.append(("end_runs", rows, {"chr3": [[990, 1100, "LINE_x"]]}, 30))
    # one element on the chromosome
    els = {"chr1": [[1000, 1050, "SINE_a"]], "chr2": [[500, 500, "dot"]]}
    rows = [("chr1", "+", 960, rnd(rng, 40)), ("chr1", "+", 976, rnd(rng, 24)), ("chr1", "+", 977, rnd(rng, 24)),
            ("chr1", "-", 1050, rnd(rng, 20)), ("chr1", "-", 1051, rnd(rng, 20)), ("chr1", "+", 1010, rnd(rng, 20)),
            ("chr2", "+", 481, rnd(rng, 20)), ("chr2", "+", 480, rnd(rng, 20)), ("chr2", "-", 500, rnd(rng, 20)),
            ("chr2", "+", 501, rnd(rng, 20)), ("chr4", "+", 1000, rnd(rng, 20))]
    rows += random_rows(rng, els, ["chr1", "chr2"], 20, [16, 20, 25, 30], 2000)
    w.append(("one_element", rows, els, 30))
    # two elements; the farther one alone intersects
    els = {"chr1": [[1000, 1010, "near"], [1100, 1150, "far"]], "chr2": [[300, 900, "wide"], [320, 330, "inner"]]}
    rows = [("chr1", "+", 1020, rnd(rng, 20)), ("chr1", "+", 1005, rnd(rng, 20)), ("chr1", "+", 1081, rnd(rng, 25)),
            ("chr1", "-", 1090, rnd(rng, 20)), ("chr1", "+", 1151, rnd(rng, 20)), ("chr1", "+", 1011, rnd(rng, 30)),
            ("chr2", "+", 325, rnd(rng, 20)), ("chr2", "+", 600, rnd(rng, 20)), ("chr2", "-", 901, rnd(rng, 20)),
            ("chr2", "+", 1, rnd(rng, 20))]
    rows += random_rows(rng, els, ["chr1", "chr2"], 20, [16, 20, 25, 30], 2000)
    w.append(("two_elements", rows, els, 30))
    # many elements; clusters before all starts and after all starts
    els = {"chr1": distinct_elements(rng, 120, 20000, "rep"), "chr7": distinct_elements(rng, 40, 3000, "L1_")}
    lo, hi = min(e[0] for e in els["chr1"]), max(e[0] for e in els["chr1"])
    rows = [("chr1", "+", 1, rnd(rng, 16)), ("chr1", "-", max(1, lo - 10), rnd(rng, 30)), ("chr1", "+", hi + 1, rnd(rng, 20)),
            ("chr1", "-", hi + 3000, rnd(rng, 20))]
    rows = [r for r in rows if tie_free(els, r[0], r[2])]
    rows += random_rows(rng, els, ["chr1", "chr7", "chrUn"], 40, [16, 18, 22, 25, 30, 31], 21000)
    w.append(("many_elements", rows, els, 30))
    # elements with end < start cover nothing
    els = {"chr1": [[1000, 900, "backwards"], [1200, 1199, "empty"], [1500, 1510, "real"]]}
    rows = [("chr1", "+", 990, rnd(rng, 20)), ("chr1", "+", 950, rnd(rng, 20)), ("chr1", "-", 1195, rnd(rng, 20)),
            ("chr1", "+", 1495, rnd(rng, 20)), ("chr1", "+", 1360, rnd(rng, 20))]
    rows += random_rows(rng, els, ["chr1"], 12, [16, 20, 25], 2000)
    w.append(("end_before_start", rows, els, 30))
    # a long element covers the cluster but two others start nearer: the reference does not see it
    els = {"chr1": [[100, 9000, "giant"], [4000, 4005, "s1"], [4100, 4110, "s2"], [4300, 4310, "s3"]]}
    rows = [("chr1", "+", 4040, rnd(rng, 20)), ("chr1", "-", 4220, rnd(rng, 20)), ("chr1", "+", 4001, rnd(rng, 20)),
            ("chr1", "+", 500, rnd(rng, 20)), ("chr1", "+", 2040, rnd(rng, 20)), ("chr1", "-", 8000, rnd(rng, 20)),
            ("chr1", "+", 4160, rnd(rng, 25)), ("chr1", "-", 4311, rnd(rng, 16)), ("chr1", "+", 90, rnd(rng, 20))]
    rows += random_rows(rng, els, ["chr1"], 12, [16, 20, 25], 9500)
    w.append(("long_cover", rows, els, 30))
    # everything at once under other cutoffs
    for name, cutoff in (("mixed_25", 25), ("mixed_18", 18)):
        els = {"chr1": distinct_elements(rng, 60, 6000, "a"), "chr2": distinct_elements(rng, 2, 6000, "b"),
               "chr3": distinct_elements(rng, 1, 6000, "c"), "chr9": distinct_elements(rng, 5, 6000, "unused")}
        rows = random_rows(rng, els, ["chr1", "chr2", "chr3", "chr5"], 36, [16, 17, 18, 19, 24, 25, 26, 30], 6500)
        rows += [("chr1", "+", 77, "C" * 10 + "A" * 6), ("chr2", "-", 78, "T" * 7 + "C" * 10)]
        rows = [r for r in rows if tie_free(els, r[0], r[2])]
        w.append((name, rows, els, cutoff))
    w.append(("empty", [], {"chr1": [[1, 10, "x"]]}, 30))
    return w


def ties_world():
    rng = np.random.default_rng(77)
    els = {"chr1": [[1000, 1060, "a"], [1000, 1005, "b"], [1100, 1100, "c"],          # equal starts, equal distance at 1050
                    [3000, 3004, "d"], [3100, 3190, "e"], [3000, 3150, "f"], [3000, 3001, "g"]],
           "chr2": [[500, 520, "h"], [600, 640, "i"], [700, 705, "j"]]}               # 550 and 650 are equidistant
    rows = [("chr1", "+", 1050, rnd(rng, 20)), ("chr1", "+", 3050, rnd(rng, 20)), ("chr2", "+", 650, rnd(rng, 20)),
            ("chr2", "-", 550, rnd(rng, 25))]
    rows += random_rows(rng, els, ["chr1", "chr2"], 44, [16, 20, 25, 30, 31], 4000)
    return "ties", rows, els, 30


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    tmp, trim, gen = load_reference(sys.argv[1])
    out = []
    try:
        for k, (name, rows, els, cutoff) in enumerate(worlds() + [ties_world()]):
            text = table(rows)
            ties = name == "ties"
            if not ties:
                assert all(tie_free(els, r[0], r[2]) for r in rows), name
                assert model.outcomes(text, els, cutoff) == model.outcomes(text, els, cutoff, high_first=True), name
            path = os.path.join(tmp, "w%d_vs_genome_sorted_clusters.tsv" % k)
            with open(path, "w") as fh:
                fh.write(text)
            trim(coordinate_dic(els), path, str(cutoff))
            gen(path[:-4] + "_trimmed.tsv")
            got = [open(path[:-4] + sfx).read() for sfx in ("_trimmed.tsv", "_trimmed.fa", "_trimmed_orig.fa")]
            out.append(dict(name=name, ties=ties, cutoff=cutoff, table=text, elements=els, trimmed_tsv=got[0], trimmed_fa=got[1],
                            trimmed_orig_fa=got[2]))
            print("%-18s %3d clusters, %3d retained" % (name, len(rows), got[1].count(">")))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    with open(OUT, "w") as fh:
        json.dump(dict(source="reference utils/preTrimClusteredSeq.py + utils/generate_Seq.py", worlds=out), fh, indent=0)
    print("wrote %s: %d worlds, %d bytes" % (OUT, len(out), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
