#!/usr/bin/env python3
"""Capture tests/golden/predict_remap.json from the REFERENCE's own split_fasta_from_sam, combineSam, decorateSam and
parse_refine_sam (utils/processSam.py) and `LC_ALL=C sort -k6,6 -k1,1`, strung together as miRge2.0.py:566-601 does.

    python tests/golden/make_predict_remap_golden.py <reference src/mirge directory>

Run only in the build container: processSam.py is copied to a scratch directory outside the repository, CRLF stripped,
converted with lib2to3, and imported from there next to a ten-line stand-in for Bio.SeqIO.parse, which this script writes
into that directory.  Only data is written into the repository: per world the `_clusters_trimmed_orig.fa` text, the reads'
FASTA text, seedLength and the final sorted table.

bowtie is not on the machine.  The two SAM texts therefore do NOT come from bowtie: they come from
tests/bowtie_text_model.run on the two argv of the reference (`-f -n 0 -l <seedLength> -S -a --best --norc` and
`-f -n 1 -l 15 -5 1 -3 3 -S -a --best --strata --norc`).  So the reference pins split, combine, decorate, select and sort,
and the project's existing bowtie contract (which prints FLAG 0 for every forward alignment)
pins the SAM lines.

The worlds are seeded; properties() names what they must hold together and main() asserts that each occurs, so a world
cannot lose its case silently.
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
import bowtie_text_model as btm  # noqa: E402
import predict_remap_model as model  # noqa: E402

OUT = os.path.join(HERE, "predict_remap.json")
SEQIO = '''class _Record(object):
    def __init__(self, id):
        self.id, self.seq = id, ""


def parse(path, fmt):
    rec = None
    for line in open(path):
        line = line.strip()
        if line.startswith(">"):
            if rec is not None:
                yield rec
            rec = _Record(line[1:].split()[0])
        elif line and rec is not None:
            rec.seq += line
    if rec is not None:
        yield rec
'''


def load_reference(src):
    tmp = tempfile.mkdtemp(prefix="predict_remap_golden_")
    os.mkdir(os.path.join(tmp, "Bio"))
    for fn, text in (("__init__.py", ""), ("SeqIO.py", SEQIO)):
        with open(os.path.join(tmp, "Bio", fn), "w") as fh:
            fh.write(text)
    sys.path.insert(0, tmp)
    dst = os.path.join(tmp, "processSam.py")
    with open(os.path.join(src, "utils", "processSam.py"), "rb") as fh:
        data = fh.read().replace(b"\r\n", b"\n")
    with open(dst, "wb") as fh:
        fh.write(data)
    subprocess.run([sys.executable, "-m", "lib2to3", "-w", "-n", dst], capture_output=True)
    spec = importlib.util.spec_from_file_location("processSam", dst)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return tmp, mod


def rnd(rng, n):
    return "".join("ACGT"[c] for c in rng.integers(0, 4, n))


def mutate(s, i):
    i %= len(s)
    return s[:i] + "ACGT"[("ACGT".index(s[i]) + 1) % 4] + s[i + 1:]


def piece(rng, s, lo=16, hi=25):
    n = int(rng.integers(lo, min(hi, len(s)) + 1))
    a = int(rng.integers(0, len(s) - n + 1))
    return s[a:a + n]


def world(seed, n_random):
    """(clusters [(number, sequence)], reads [sequence]) holding every case of the module's list."""
    rng = np.random.default_rng(seed)
    A = rnd(rng, 30)
    B = A[4:26] + rnd(rng, 6)                        # shares a 22-mer with A
    X = rnd(rng, 30)
    Y = mutate(X[2:28], 12)                          # X[2:28] with one base changed
    P = "ACGGTC" * 5                                 # a repeat: its 18-mers sit at three offsets
    special = [A, B, X, Y, P]
    randoms = [rnd(rng, int(rng.integers(25 if k < 13 else 16, 31))) for k in range(n_random)]   # (the cases below cut 19 .. 25 nt)
    seqs = special + randoms
    order = rng.permutation(len(seqs))
    pool = [8, 9, 10, 11] + list(range(97, 97 + len(seqs)))
    clusters = [(pool[k], seqs[int(j)]) for k, j in enumerate(order)]
    reads = []
    for s in seqs:
        reads.append(piece(rng, s))                  # exact, one cluster (mostly)
    reads += [A[4:26], A[5:25], A[8:26][:18]]         # several clusters
    reads += [rnd(rng, 25) for _ in range(5)]        # nothing
    for s in randoms[:4]:
        reads.append(mutate(piece(rng, s, 20, 25), 0))                  # pass 2 only: the cut first base differs
    for s in randoms[4:8]:
        r = piece(rng, s, 19, 19) if len(s) >= 19 else None
        if r:
            reads.append(mutate(r, len(r) - 2))                         # pass 2 only: a cut 3' base differs
    reads.append(mutate(X[3:27], 0))                 # pass 2: X exactly, Y one seed mismatch worse -> only X
    reads.append(mutate(Y[1:25], 0))                 # pass 2: Y exactly, X one worse -> only Y
    for s in randoms[8:11]:
        r = piece(rng, s, 22, 25) if len(s) >= 22 else None
        if r:
            reads.append(mutate(mutate(r, 0), 8))    # pass 2 with one seed mismatch, nothing better
    reads += ["ACGGTC" * 3, "CGGTCA" * 3]            # one cluster, three and two offsets
    for s in randoms[11:13]:
        r = piece(rng, s, 22, 25) if len(s) >= 22 else None
        if r:
            reads.append(r[:10] + "N" + r[11:])      # an N
    reads = list(dict.fromkeys(reads))               # (collapsed reads are distinct)
    reads = [reads[int(j)] for j in rng.permutation(len(reads))]
    assert len(reads) <= 100
    return clusters, reads


def fasta_texts(clusters, reads, rng):
    cl = "".join(">smp:miRCluster_%d_%d:chr%d:%d_%d%s\n%s\n" % (i, len(s), 1 + i % 3, 100 * i, 100 * i + len(s) - 1, "+-"[i % 2], s)
                 for i, s in clusters)
    numbers = ([7, 8, 9, 10, 11, 12] + list(range(90, 90 + len(reads))))[:len(reads)]
    rd = "".join(">mir%d_%d\n%s\n" % (n, int(rng.integers(2, 500)), s) for n, s in zip(numbers, reads))
    return cl, rd


def reference_table(ps, tmp, k, seed_length, cl_text, rd_text):
    """miRge2.0.py:566-601 with bowtie_text_model in bowtie's place: (table text, SAM 1, SAM 2)."""
    d = os.path.join(tmp, "w%d" % k)
    os.mkdir(d)
    reads_path = os.path.join(d, "unmapped_mirna_smp.fa")
    orig_path = os.path.join(d, "smp_clusters_trimmed_orig.fa")
    o4 = os.path.join(d, "unmapped_mirna_smp_vs_representative_seq")
    for path, text in ((reads_path, rd_text), (orig_path, cl_text)):
        with open(path, "w") as fh:
            fh.write(text)
    parts = [model.parse_fasta(cl_text)]
    sam1, _ = btm.run(model.pass1_argv(seed_length) + ["ix", reads_path], parts, rd_text)
    with open(o4 + "_tmp1.sam", "w") as fh:
        fh.write(sam1)
    ps.split_fasta_from_sam(o4 + "_tmp1.sam", reads_path)
    left = open(reads_path[:-3] + "_imperfectMath2Cluster.fa").read()
    sam2, _ = btm.run(model.PASS2_ARGV + ["ix", "left.fa"], parts, left)
    with open(o4 + "_tmp2.sam", "w") as fh:
        fh.write(sam2)
    ps.combineSam(o4 + "_tmp1.sam", o4 + "_tmp2.sam")
    ps.decorateSam(o4 + ".sam", reads_path, orig_path)
    ps.parse_refine_sam(o4 + "_modified.sam")
    with open(o4 + "_modified_selected_sorted.tsv", "w") as fh:
        subprocess.run(["sort", "-k6,6", "-k1,1", o4 + "_modified_selected.tsv"], stdout=fh, check=True,
                       env=dict(os.environ, LC_ALL="C"))
    assert open(o4 + "_modified_selected.tsv").read() == open(o4 + "_modified_selected_reverseKept.tsv").read()
    return open(o4 + "_modified_selected_sorted.tsv").read(), sam1, sam2, left


def properties(seed_length, cl_text, rd_text, table, sam1, sam2, left):
    """The names of the cases this world holds."""
    names, seqs = model.parse_fasta(rd_text)
    cnames, cseqs = model.parse_fasta(cl_text)
    seq_of, cseq_of = dict(zip(names, seqs)), dict(zip(cnames, cseqs))
    a1, a2 = model.sam_alignments(sam1), model.sam_alignments(sam2)
    rows = [f.split("\t") for f in table.splitlines()]
    by_read, by_pair = {}, {}
    for r, c, o, mm in a1 + a2:
        by_read.setdefault(r, set()).add(c)
        by_pair[(r, c)] = by_pair.get((r, c), 0) + 1
    got = {"seed_length_%d" % seed_length}
    p1 = set(r for r, _, _, _ in a1)
    if any(len(by_read[r]) == 1 and by_pair[(r, c)] == 1 and mm == 0 for r, c, o, mm in a1):
        got.add("one_cluster_exact")
    if any(len(v) > 1 for v in by_read.values()):
        got.add("several_clusters")
    if any(n not in by_read for n in names):
        got.add("no_alignment")
    for r, c, o, mm in a2:
        s, cs = seq_of[r], cseq_of[c]
        assert r not in p1
        if o >= 1 and s[0] != cs[o - 1] and mm == 0:
            got.add("pass2_first_base")
        tail = cs[o - 1 + len(s) - 3:o - 1 + len(s)]
        if o >= 1 and len(tail) == 3 and tail != s[-3:] and s[0] == cs[o - 1]:
            got.add("pass2_three_prime")
        if mm >= 1:
            got.add("pass2_seed_mismatch_row")
        if "N" in s:
            got.add("n_in_read")
    w = btm.World([(cnames, cseqs)])
    for n, s in zip(*model.parse_fasta(left)):
        hs = w.hits(model.trim(s), (15, 1, 2), True, 65536)
        if len(set(h[0] for h in hs)) > 1:
            listed = [a for a in a2 if a[0] == n]
            assert listed and len(listed) < len(hs) and len(set(a[3] for a in listed)) == 1
            got.add("better_stratum_competitor")
    if any(v > 1 for v in by_pair.values()):
        got.add("two_offsets_one_cluster")
    cn = sorted(set(model.cluster_number(f[5]) for f in rows))
    if sorted(cn, key=lambda i: str(i) + "_") != cn and {9, 10, 99, 100} <= set(cn):
        got.add("cluster_numbers_cross")
    for c in set(f[5] for f in rows):
        rn = sorted(set(model.read_number(f[0]) for f in rows if f[5] == c))
        if sorted(rn, key=lambda i: str(i) + "_") != rn:
            got.add("read_numbers_cross")
    rn = set(model.read_number(f[0]) for f in rows)
    if not ({9, 10} <= rn and {99, 100} <= rn):
        got.discard("read_numbers_cross")
    if not rows:
        got.add("empty_result")
    return got


WANTED = {"seed_length_25", "seed_length_18", "one_cluster_exact", "several_clusters", "no_alignment", "pass2_first_base",
          "pass2_three_prime", "pass2_seed_mismatch_row", "better_stratum_competitor", "two_offsets_one_cluster", "cluster_numbers_cross",
          "read_numbers_cross", "n_in_read", "empty_result"}


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    tmp, ps = load_reference(sys.argv[1])
    out, seen = [], set()
    try:
        rng = np.random.default_rng(5660)
        specs = [("sl25", 25, world(101, 22)), ("sl18", 18, world(202, 18)),
                 ("empty", 25, ([(i + 1, rnd(rng, 24)) for i in range(10)], [rnd(rng, 25) for _ in range(8)]))]
        for k, (name, sl, (clusters, reads)) in enumerate(specs):
            cl_text, rd_text = fasta_texts(clusters, reads, rng)
            table, sam1, sam2, left = reference_table(ps, tmp, k, sl, cl_text, rd_text)
            got = properties(sl, cl_text, rd_text, table, sam1, sam2, left)
            mine, _ = model.table_from_sam(sam1, sam2, rd_text, cl_text)
            assert mine == table, "%s: the model and the reference disagree" % name
            seen |= got
            out.append(dict(name=name, seed_length=sl, clusters_fa=cl_text, reads_fa=rd_text, table=table, holds=sorted(got)))
            print("%-6s %3d clusters, %3d reads, %3d lines: %s" % (name, len(clusters), len(reads), table.count("\n"), " ".join(sorted(got))))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    missing = WANTED - seen
    assert not missing, "no world holds: %s" % " ".join(sorted(missing))
    with open(OUT, "w") as fh:
        json.dump(dict(source="reference utils/processSam.py + `LC_ALL=C sort -k6,6 -k1,1`; SAM text from tests/bowtie_text_model.run",
                       worlds=out), fh, indent=0)
    print("wrote %s: %d worlds, %d bytes" % (OUT, len(out), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
