#!/usr/bin/env python3
"""Capture tests/golden/predict_features.json from the REFERENCE's own utils/generate_featureFiles.py and
classes/readCluster.py (miRge2.0.py:604).

    python tests/golden/make_predict_features_golden.py <reference src/mirge directory>

Run only in the build container: the two modules are copied to a scratch directory outside the repository, CRLF stripped,
converted with lib2to3 and imported from there next to stand-ins for Bio.Seq, Bio.SeqIO, Bio.Alphabet and Bio.pairwise2,
which this script writes into that directory.  `pairwise2.align.localms` is answered by the generator's own
pairwise2_localms (tests/golden/make_golden.py), not by product code.  The capture runs under Python 3, whose str(float)
is not Python 2's, so the two imported modules get a module-global `str` that prints a float as Python 2.7 does (%.12g,
`.0` appended when neither `.` nor `e` shows) and hands everything else to the builtin.

Only data is written into the repository: per world the table's name and text, the chromosomes and the two files.  The
input tables are built with tests/predict_remap_model.table from chosen rows.  The worlds are seeded; WANTED names what
they must hold together and main() asserts that each case occurs, so a world cannot lose its case silently.
"""
import builtins
import importlib.util
import json
import os
import shutil
import subprocess
import sys
import tempfile
from fractions import Fraction

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import predict_features_model as model  # noqa: E402
import predict_remap_model as prm  # noqa: E402

OUT = os.path.join(HERE, "predict_features.json")
STEM = "_vs_representative_seq_modified_selected_sorted.tsv"
STANDINS = {
    "Bio/__init__.py": "",
    "Bio/SeqIO.py": "",
    "Bio/Alphabet/__init__.py": "IUPAC = Gapped = generic_dna = None\n",
    "Bio/Seq.py": '''class Seq(object):
    def __init__(self, data, alphabet=None):
        self.data = data

    def reverse_complement(self):
        return Seq(self.data.translate(str.maketrans("ACGT", "TGCA"))[::-1])

    def __str__(self):
        return self.data
''',
    "Bio/pairwise2.py": '''class _Align(object):
    localms = None


align = _Align()
''',
    "mirge/__init__.py": "",
    "mirge/classes/__init__.py": "",
}


def py2_str(x):
    if isinstance(x, float):
        s = "%.12g" % x
        return s if ("." in s or "e" in s or "n" in s) else s + ".0"
    return builtins.str(x)


def load_module(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def load_reference(src):
    tmp = tempfile.mkdtemp(prefix="predict_features_golden_")
    for rel, text in STANDINS.items():
        os.makedirs(os.path.dirname(os.path.join(tmp, rel)), exist_ok=True)
        with open(os.path.join(tmp, rel), "w") as fh:
            fh.write(text)
    copies = (("classes/readCluster.py", "mirge/classes/readCluster.py"), ("utils/generate_featureFiles.py", "generate_featureFiles.py"))
    for rel, to in copies:
        with open(os.path.join(src, rel), "rb") as fh:
            data = fh.read().replace(b"\r\n", b"\n")
        with open(os.path.join(tmp, to), "wb") as fh:
            fh.write(data)
        subprocess.run([sys.executable, "-m", "lib2to3", "-w", "-n", os.path.join(tmp, to)], capture_output=True, check=True)
    sys.path.insert(0, tmp)
    golden = load_module("make_golden_for_localms", os.path.join(HERE, "make_golden.py"))
    import Bio.pairwise2
    Bio.pairwise2.align.localms = staticmethod(golden.pairwise2_localms)
    import mirge.classes.readCluster as rc
    gf = load_module("generate_featureFiles", os.path.join(tmp, "generate_featureFiles.py"))
    rc.str = gf.str = py2_str
    return tmp, gf


def rnd(rng, n):
    return "".join("ACGT"[c] for c in rng.integers(0, 4, n))


def other(base, step=1):
    return "ACGT"[("ACGT".index(base) + step) % 4]


class World:
    """Chromosomes, clusters cut from them, reads and chosen rows; text() is the sorted table."""

    def __init__(self, seed, chrom_lens, name="unmapped_mirna_smp"):
        self.rng = np.random.default_rng(seed)
        self.name = name + STEM
        self.chroms = {ch: rnd(self.rng, n) for ch, n in chrom_lens}
        self.cnames, self.cseqs, self.cnumbers = [], [], []
        self.reads, self.counts, self.rows = [], [], []
        self.next_cluster = 7          # (numbers 7 .. 12 and 97 .. cross the byte order of their digits)

    def patch(self, ch, at, text):
        """chromosome[at - 1 ...] = text (1-based)."""
        s = self.chroms[ch]
        self.chroms[ch] = s[:at - 1] + text + s[at - 1 + len(text):]

    def cluster(self, ch, start, length, strand="+"):
        s = self.chroms[ch][start - 1:start - 1 + length].upper()
        if strand == "-":
            s = model.revcomp(s)
        k = self.next_cluster
        self.next_cluster = 97 if k == 12 else k + 1
        self.cnames.append("smp:miRCluster_%d_%d:%s:%d_%d%s" % (k, length, ch, start, start + length - 1, strand))
        self.cseqs.append(s)
        self.cnumbers.append(k)
        return len(self.cseqs) - 1

    def read(self, seq, count):
        self.reads.append(seq)
        self.counts.append(count)
        return len(self.reads) - 1

    def member(self, c, count, a=0, b=None, mut=(), pre=None, post=None, offsets=None):
        """One read on cluster c: cluster[a:b] with the positions `mut` (position, step) changed; pre / post (1 and 3 bases)
        make it a pass-2 row, whose cut bases they are.  offsets: list the read at these offsets (default: a)."""
        s = list(self.cseqs[c][a:b])
        for p, step in mut:
            s[p] = other(s[p], step)
        s = "".join(s)
        second = pre is not None
        r = self.read((pre + s + post) if second else s, count)
        for o in (offsets or [a]):
            self.rows.append((r, c, o, len(mut), 1 if second else 0))
        return r

    def text(self):
        numbers = ([8, 9, 10, 11] + list(range(95, 95 + len(self.reads))))[:len(self.reads)]
        names = ["mir%d_%d" % (n, c) for n, c in zip(numbers, self.counts)]
        rows = prm.sort_rows(self.rows, numbers, self.cnumbers)
        return prm.table(rows, names, self.reads, self.cnames, self.cseqs)


def plain(w, c, counts=(8, 1, 1)):
    """counts[0] whole-cluster reads and two shorter ones inside: every column stable, head 0, tail -1."""
    n = len(w.cseqs[c])
    w.member(c, counts[0])
    for k, cnt in enumerate(counts[1:]):
        w.member(c, cnt, 1 + k, n - 1 - k)


def main_world():
    w = World(4242, [("chr1", 300), ("chr2", 200), ("chr3", 200), ("chr4", 200), ("chr5", 200), ("chr6", 200), ("chr7", 200),
                     ("chr8", 200), ("chr9", 200), ("chr10", 200), ("chr11", 200), ("chr12", 200), ("chr13", 260)])
    # chr1: four groups at distances 9, 44 and 45; chr2: two at distance 8; chr13: +/- neighbours inside 9 .. 44, then 44 on -
    at = 30
    for gap in (9, 44, 45, None):
        plain(w, w.cluster("chr1", at, 22))
        at += 22 + (gap or 0)
    plain(w, w.cluster("chr2", 40, 20))
    plain(w, w.cluster("chr2", 40 + 20 + 8, 24))
    plain(w, w.cluster("chr13", 30, 20, "+"))
    plain(w, w.cluster("chr13", 30 + 20 + 20, 20, "-"))
    plain(w, w.cluster("chr13", 70 + 20 + 44, 21, "-"))
    # chr3: the filter's passing edges (start 21, count sum 10, three members; end one below chrLen - 20)
    plain(w, w.cluster("chr3", 21, 20), (8, 1, 1))
    plain(w, w.cluster("chr3", 200 - 21 - 21 + 1, 21), (20, 3, 2))
    # chr4: the failing edges -- nothing survives there
    plain(w, w.cluster("chr4", 20, 20))                          # start 20
    plain(w, w.cluster("chr4", 200 - 20 - 22 + 1, 22))          # end = chrLen - 20
    plain(w, w.cluster("chr4", 60, 20), (7, 1, 1))               # count sum 9
    c = w.cluster("chr4", 100, 20)
    w.member(c, 30)
    w.member(c, 5, 1, 19)                                        # two members
    # chr5: pass-2 members overhanging at the head and at the tail, their cut bases mismatching; an N in the genome under
    # the second overhanging column
    c = w.cluster("chr5", 50, 24)
    w.patch("chr5", 50 + 24 + 1, "N")
    w.member(c, 12)
    before = w.chroms["chr5"][48]
    w.member(c, 2, 0, 20, pre=other(before), post="".join(other(x) for x in w.cseqs[c][20:23]))
    after = w.chroms["chr5"][73:76]
    w.member(c, 1, 3, 24, pre=other(w.cseqs[c][2]), post=other(after[0]) + "A" + other(after[2], 2))
    # chr6: a cluster of repeats: one read listed at two offsets, its alignment tied between diagonals
    w.patch("chr6", 60, "ACGGTC" * 4)
    c = w.cluster("chr6", 60, 24)
    w.member(c, 9)
    w.member(c, 2, 0, 18, offsets=[0, 6])
    w.member(c, 1, 2, 22)
    # chr7: ratios 12/15 = 4/5 (stable) at column 0 and 14/18-like 7/9 inside is below; here 4/5 in the FIRST column
    c = w.cluster("chr7", 40, 22)
    w.member(c, 12)
    w.member(c, 2, mut=[(0, 1)])
    w.member(c, 1, mut=[(0, 2)])
    # chr8: 7/9 in the first column (unstable: head = 1) and 8/10 in the last
    c = w.cluster("chr8", 40, 22, "-")
    w.member(c, 14)
    w.member(c, 2, mut=[(0, 1)])
    w.member(c, 2, mut=[(0, 1)], a=0, b=21)
    c = w.cluster("chr8", 120, 20)
    w.member(c, 8)
    w.member(c, 1, mut=[(19, 1)])
    w.member(c, 1, mut=[(19, 2)])
    # chr9: two bases tied in a column (5 : 5 : 1), and a group without a stable column
    c = w.cluster("chr9", 30, 22)
    w.member(c, 5)
    w.member(c, 5, mut=[(10, 2)])
    w.member(c, 1, 11, 22)
    c = w.cluster("chr9", 120, 20)
    w.member(c, 4, 0, 8)
    w.member(c, 4, 6, 14)
    w.member(c, 4, 12, 20)
    # chr10: head 4 and tailAdd 7: stable length 18 - 4 - 7 = 7 (written); chr11: head 5: 6 (not written)
    for ch, head in (("chr10", 4), ("chr11", 5)):
        c = w.cluster(ch, 60, 18)
        w.member(c, 12, head, 11)
        w.member(c, 1)
        w.member(c, 1, 1, 18)
    # chr12: a member with an N
    c = w.cluster("chr12", 50, 22)
    w.member(c, 10)
    w.member(c, 3, 1, 21)
    r = w.member(c, 2, 2, 22)
    w.reads[r] = w.reads[r][:7] + "N" + w.reads[r][8:]
    return w


def mapped_world():
    w = World(777, [("chr2", 150), ("chrX", 150)], name="mapped_nonmirna_smp")
    plain(w, w.cluster("chr2", 40, 20), (30, 4, 2))
    plain(w, w.cluster("chrX", 50, 25, "-"), (9, 9, 9))
    return w


def empty_world():
    w = World(31, [("chr1", 120)])
    plain(w, w.cluster("chr1", 40, 20), (3, 2, 1))
    plain(w, w.cluster("chr1", 80, 20), (100, 1))
    return w


def reference_files(gf, tmp, k, w):
    d = os.path.join(tmp, "w%d" % k)
    os.mkdir(d)
    path = os.path.join(d, w.name)
    with open(path, "w") as fh:
        fh.write(w.text())
    gf.generate_featureFiles(path, w.chroms, {ch: len(s) for ch, s in w.chroms.items()}, {}, {})
    return open(path[:-4] + "_features.tsv").read(), open(path[:-4] + "_cluster.txt").read()


def properties(w, info, features):
    got = set()
    chroms, by_chr = model.parse(w.text())
    for ch in chroms:
        n = len(w.chroms[ch])
        for g in by_chr[ch]:
            total, members = sum(g[6]), len(g[5])
            ok = model.passes(g, n)
            for cond, name in ((total == 9 and not ok, "sum_9"), (total == 10 and ok, "sum_10"), (members == 2 and not ok, "members_2"),
                               (members == 3 and ok, "members_3"), (g[0] == 20 and not ok, "start_20"), (g[0] == 21 and ok, "start_21"),
                               (g[1] == n - 20 and not ok, "end_at_limit"), (g[1] == n - 21 and ok, "end_below_limit"),
                               (len(set(zip(g[4], g[5]))) < members, "member_twice")):
                if cond:
                    got.add(name)
            if any("N" in s for s in g[5]) and ok:
                got.add("member_with_n")
    per_chr = {}
    for d in info["groups"]:
        rows, counts = d["rows"], d["counts"]
        if d["H"] > 0 and d["T"] > 0:
            got.add("overhang_head_and_tail")
        if d["head"] is None:
            got.add("no_stable_column")
            continue
        per_chr.setdefault(d["chr"], []).append(d)
        for i in range(len(rows[0])):
            t = model.tallies(rows, counts, i)
            best = sorted((t[b] for b in model.BASES), reverse=True)
            f = Fraction(best[0], d["total"])
            if f == Fraction(4, 5) and d["total"] != 10:
                got.add("ratio_4_5")
            if best[0] == 8 and d["total"] == 10:
                got.add("ratio_8_10")
            if f == Fraction(7, 9):
                got.add("ratio_7_9")
            if best[0] == best[1] > 0:
                got.add("column_tie")
        got.add("head_below_3" if d["head"] < 3 else "head_from_3")
        tail_add = -d["tail"] - 1
        got.add("tail_add_below_6" if tail_add < 6 else "tail_add_from_6")
        _, pad_h, pad_t = model.feature_columns(len(rows[0]), d["head"], d["tail"])
        stable = len(rows[0]) + pad_h + pad_t - d["head"] - tail_add
        if stable in (6, 7):
            assert d["written"] == (stable == 7)
            got.add("stable_length_%d" % stable)
        if d["strand"] == "-":
            got.add("minus_cluster")
        cols, pad_h, _ = model.feature_columns(len(rows[0]), d["head"], d["tail"])
        if any(d["template"][x + pad_h] not in model.BASES for x in cols[1:]) and d["template"][cols[0] + pad_h] in model.BASES:
            got.add("template_n_later_column")
        for dist in (d["up"], d["down"]):
            if dist in (8, 9, 44, 45):
                got.add("distance_%d" % dist)
    for ch, ds in per_chr.items():
        if len(ds) in (1, 2, 4):
            got.add("chromosome_with_%d" % len(ds))
        for a, b in zip(ds, ds[1:]):
            if a["strand"] != b["strand"] and 9 <= a["down"] <= 44:
                got.add("unequal_strands")
    names = [ch for ch in chroms if ch in per_chr]
    if "chr10" in names and "chr2" in names and names.index("chr10") < names.index("chr2"):
        got.add("chr10_before_chr2")
    # a pass-2 style member whose cut bases mismatch the genome beside its alignment
    for r, c, o, mm, p in w.rows:
        if p:
            ch, start, end, strand = model.name_fields(w.cnames[c])
            if strand == "+" and o == 0 and w.reads[r][0] != w.chroms[ch][start - 2]:
                got.add("pass2_cut_mismatch")
    # a tie between diagonals: the best ungapped score of a (cluster, read) pair ends in several cells
    for r, c, o, mm, p in w.rows:
        cs, s = w.cseqs[c], w.reads[r]
        best = {}
        for d0 in range(-len(s) + 1, len(cs)):
            run = top = 0
            for i in range(len(s)):
                j = d0 + i
                if 0 <= j < len(cs):
                    run = max(0, run + (2 if cs[j] == s[i] else -1))
                    top = max(top, run)
            best[d0] = top
        m = max(best.values())
        if sum(1 for v in best.values() if v == m) > 1:
            got.add("tied_alignment")
    if os.path.basename(w.name).startswith("mapped_"):
        got.add("mapped_name")
        assert all(ln.startswith("-1\tNull\t") for ln in features.splitlines()[1:])
    if info["passed"] == 0:
        got.add("no_surviving_group")
        assert features == model.HEADER_HEAD
    return got


WANTED = {"sum_9", "sum_10", "members_2", "members_3", "start_20", "start_21", "end_at_limit", "end_below_limit",
          "overhang_head_and_tail", "pass2_cut_mismatch", "member_twice", "ratio_4_5", "ratio_7_9", "ratio_8_10", "column_tie",
          "no_stable_column", "head_below_3", "head_from_3", "tail_add_below_6", "tail_add_from_6", "minus_cluster",
          "stable_length_6", "stable_length_7", "chromosome_with_1", "chromosome_with_2", "chromosome_with_4", "distance_8",
          "distance_9", "distance_44", "distance_45", "unequal_strands", "chr10_before_chr2", "template_n_later_column",
          "tied_alignment", "member_with_n", "mapped_name", "no_surviving_group"}


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    tmp, gf = load_reference(sys.argv[1])
    out, seen = [], set()
    try:
        for k, (name, w) in enumerate((("main", main_world()), ("mapped", mapped_world()), ("empty", empty_world()))):
            features, cluster = reference_files(gf, tmp, k, w)
            mine_f, mine_c, info = model.run(w.text(), w.chroms, w.name)
            assert mine_f == features, "%s: the model's _features.tsv and the reference's disagree" % name
            assert mine_c == cluster, "%s: the model's _cluster.txt and the reference's disagree" % name
            got = properties(w, info, features)
            seen |= got
            out.append(dict(name=name, table_name=w.name, table=w.text(), chromosomes=w.chroms, features=features, cluster=cluster,
                            holds=sorted(got)))
            print("%-6s %3d lines, %2d groups pass, %2d feature lines: %s" % (name, w.text().count("\n"), info["passed"],
                                                                             features.count("\n") - 1, " ".join(sorted(got))))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    missing = WANTED - seen
    assert not missing, "no world holds: %s" % " ".join(sorted(missing))
    with open(OUT, "w") as fh:
        json.dump(dict(source="reference utils/generate_featureFiles.py + classes/readCluster.py under lib2to3; localms from "
                              "make_golden.pairwise2_localms; tables from tests/predict_remap_model.table", worlds=out), fh, indent=0)
    print("wrote %s: %d worlds, %d bytes" % (OUT, len(out), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
