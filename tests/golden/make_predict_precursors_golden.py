#!/usr/bin/env python3
"""Capture tests/golden/predict_precursors.json from the REFERENCE's own utils/get_precursors.py (miRge2.0.py:608) and
utils/renameStrFile.py.

    python tests/golden/make_predict_precursors_golden.py <reference src/mirge directory>

Run only in the build container: the two modules are copied to a scratch directory outside the repository, CRLF stripped,
converted with lib2to3 and imported from there next to stand-ins for Bio.Seq (Seq with reverse_complement, transcribe and
__str__) and Bio.Alphabet, which this script writes into that directory.  The worlds hold upper-case A, C, G, T and N only:
there the stand-in and Biopython cannot differ (both map A<->T and C<->G, leave N, reverse, and turn T into U).

Only data is written into the repository: per world the feature table's text, the chromosomes and the text of
`_features_precusor.fa`; and one pair for renameStrFile -- a FASTA, an RNAfold-shaped text written by hand (no RNAfold is
run) and the function's output.  The three worlds of predict_features.json come with their `features` text and chromosomes;
the lines of the world `hand` are written here, WANTED names what they must hold and main() asserts every case, so the
world cannot lose one silently.
"""
import importlib.util
import json
import os
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import predict_features_model as features_model  # noqa: E402
import predict_precursors_model as model  # noqa: E402

OUT = os.path.join(HERE, "predict_precursors.json")
FEATURES = os.path.join(HERE, "predict_features.json")
TABLE = "unmapped_mirna_smp_vs_representative_seq_modified_selected_sorted_features.tsv"
STANDINS = {
    "Bio/__init__.py": "",
    "Bio/Alphabet/__init__.py": "generic_dna = None\n",
    "Bio/Seq.py": '''class Seq(object):
    def __init__(self, data, alphabet=None):
        self.data = data

    def reverse_complement(self):
        return Seq(self.data.translate(str.maketrans("ACGT", "TGCA"))[::-1])

    def transcribe(self):
        return Seq(self.data.replace("T", "U"))

    def __str__(self):
        return self.data
''',
}
HEADER = features_model.HEADER_HEAD + features_model.HEADER_TAIL
COLUMNS = HEADER.rstrip("\n").split("\t")


def load_reference(src):
    tmp = tempfile.mkdtemp(prefix="predict_precursors_golden_")
    for rel, text in STANDINS.items():
        os.makedirs(os.path.dirname(os.path.join(tmp, rel)), exist_ok=True)
        with open(os.path.join(tmp, rel), "w") as fh:
            fh.write(text)
    mods = []
    sys.path.insert(0, tmp)
    for name in ("get_precursors", "renameStrFile"):
        with open(os.path.join(src, "utils", name + ".py"), "rb") as fh:
            data = fh.read().replace(b"\r\n", b"\n")
        path = os.path.join(tmp, name + ".py")
        with open(path, "wb") as fh:
            fh.write(data)
        subprocess.run([sys.executable, "-m", "lib2to3", "-w", "-n", path], capture_output=True, check=True)
        spec = importlib.util.spec_from_file_location(name, path)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        mods.append(mod)
    return tmp, mods[0], mods[1]


def rnd(seed, n):
    x, out = seed, []
    for _ in range(n):
        x = (x * 6364136223846793005 + 1442695040888963407) % (1 << 64)
        out.append("ACGT"[(x >> 33) & 3])
    return "".join(out)


def line(ch, start, end, strand, H=0, T=0, hu=0, tu=0, number=7):
    """One line of `_features.tsv` with the four columns get_precursors reads; the others hold a dot."""
    f = ["."] * len(COLUMNS)
    f[5] = "smp:miRCluster_%d_%d:%s:%d_%d%s" % (number, end - start + 1, ch, start, end, strand)
    f[COLUMNS.index("alignedClusterSeq")] = "-" * H + "A" * (end - start + 1) + "-" * T
    f[COLUMNS.index("headUnstableLength")] = str(hu)
    f[COLUMNS.index("tailUnstableLength")] = str(tu)
    return "\t".join(f) + "\n"


def hand_world():
    """chr2 (400 nt, N runs at [200, 210) and [300, 320), 0-based) stands before chr10 (300 nt) in the index and behind it
    among the sorted names; the lines come in the feature file's order, chr10 first."""
    c2 = list(rnd(11, 400))
    c2[200:210] = "N" * 10
    c2[300:320] = "N" * 20
    chroms = {"chr2": "".join(c2), "chr10": rnd(12, 300)}
    rows = [
        line("chr10", 120, 141, "+", number=7),
        line("chr10", 120, 141, "-", number=8),
        line("chr10", 150, 170, "+", H=2, T=3, hu=1, tu=2, number=9),
        line("chr10", 150, 170, "-", H=1, T=2, hu=2, tu=1, number=10),
        line("chr10", 40, 60, "+", number=11),            # s - 71 < 0 <= s - 21
        line("chr10", 15, 36, "-", number=12),            # both windows clamped at 0
        line("chr10", 240, 260, "+", number=97),          # e + 70 beyond the end, e + 20 inside
        line("chr10", 270, 290, "-", number=98),          # both beyond
        line("chr2", 230, 250, "+", number=99),           # precusor_1 = [159, 270) holds the run [200, 210)
        line("chr2", 270, 290, "-", number=100),          # precusor_1 ends at 310, inside [300, 320)
        line("chr2", 381, 395, "+", number=101),          # precusor_1 starts at 310, inside [300, 320)
    ]
    return HEADER + "".join(rows), chroms


def properties(features, chroms):
    got = set()
    names = list(chroms)
    if names != sorted(names):
        got.add("index_order_is_not_name_order")
    if not model.lines(features):
        got.add("empty_table")
    for (name, ch, strand, s, e), text in zip(model.lines(features), features.split("\n")[1:]):
        f = text.split("\t")
        H, T = model.dashes(f[COLUMNS.index("alignedClusterSeq")])
        hu, tu = int(f[COLUMNS.index("headUnstableLength")]), int(f[COLUMNS.index("tailUnstableLength")])
        sign = "plus" if strand == "+" else "minus"
        got.add(sign)
        if H > 0 and T > 0:
            got.add("overhang_" + sign)
        if hu > 0 and tu > 0:
            got.add("unstable_" + sign)
        n = len(chroms[ch])
        if s - 71 < 0 <= s - 21:
            got.add("first_clamped_at_0")
        if s - 21 < 0:
            got.add("both_clamped_at_0")
        if e + 70 > n >= e + 20:
            got.add("second_beyond_end")
        if e + 20 > n:
            got.add("both_beyond_end")
        for lo, hi in model.windows(s, e, n):
            seq = chroms[ch]
            if "N" in seq[lo:hi] and seq[lo] != "N" and seq[hi - 1] != "N":
                got.add("n_run_inside")
            if hi > lo and seq[lo] == "N":
                got.add("starts_in_n_run")
            if hi > lo and seq[hi - 1] == "N":
                got.add("ends_in_n_run")
    return got


WANTED = {"plus", "minus", "overhang_plus", "overhang_minus", "unstable_plus", "unstable_minus", "first_clamped_at_0",
          "both_clamped_at_0", "second_beyond_end", "both_beyond_end", "n_run_inside", "starts_in_n_run", "ends_in_n_run",
          "index_order_is_not_name_order", "empty_table"}

# an RNAfold-shaped text: per record the name RNAfold cut at its 42nd character, the sequence, the structure and energy
RENAME_FASTA = (">smp:miRCluster_7_22:chr10:120_141+:precusor_1\nGGAUCCAUUGCACUCCGGAUGG\n"
                ">smp:miRCluster_7_22:chr10:120_141+:precusor_2\nACGGAUCCAUUGCACUCCGGAUGGCA\n"
                ">smp:miRCluster_100_21:chr2:270_290-:precusor_1\nUUGCAANNGCAA\n")
RENAME_STR = (">smp:miRCluster_7_22:chr10:120_141+:precus\nGGAUCCAUUGCACUCCGGAUGG\n.((((((.......)))))).. ( -5.40)\n"
              ">smp:miRCluster_7_22:chr10:120_141+:precus\nACGGAUCCAUUGCACUCCGGAUGGCA\n...((((((.......)))))).... ( -5.40)\n"
              ">smp:miRCluster_100_21:chr2:270_290-:precu\nUUGCAANNGCAA\n((((....)))) ( -1.10)\n")


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    tmp, gp, rn = load_reference(sys.argv[1])
    worlds = [(w["name"], w["features"], w["chromosomes"]) for w in json.load(open(FEATURES))["worlds"]]
    worlds.append(("hand",) + hand_world())
    worlds.append(("hand_empty", HEADER, {"chr1": rnd(13, 100)}))
    out, seen = [], set()
    try:
        for k, (name, features, chroms) in enumerate(worlds):
            assert all(set(s) <= set("ACGTN") for s in chroms.values()), "%s: a base other than upper-case A, C, G, T, N" % name
            d = os.path.join(tmp, "w%d" % k)
            os.mkdir(d)
            path = os.path.join(d, TABLE)
            with open(path, "w") as fh:
                fh.write(features)
            gp.get_precursors(path, chroms)
            fasta = open(path[:-4] + model.SUFFIX).read()
            assert model.run(features, chroms) == fasta, "%s: the model's file and the reference's disagree" % name
            got = properties(features, chroms)
            seen |= got
            out.append(dict(name=name, features=features, chromosomes=chroms, precursors=fasta, holds=sorted(got)))
            print("%-10s %3d lines, %3d records: %s" % (name, len(model.lines(features)), fasta.count(">"), " ".join(sorted(got))))
        for case in sorted(WANTED):
            assert case in seen, "no world holds: %s" % case
        names = [os.path.join(tmp, n) for n in ("in.fa", "in.str", "out.str")]
        for p, text in zip(names, (RENAME_FASTA, RENAME_STR)):
            with open(p, "w") as fh:
                fh.write(text)
        rn.renameStrFile(*names)
        renamed = open(names[2]).read()
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    with open(OUT, "w") as fh:
        json.dump(dict(source="reference utils/get_precursors.py and utils/renameStrFile.py under lib2to3; Bio.Seq stood in for "
                              "(upper-case A, C, G, T, N only)", worlds=out,
                       rename=dict(fasta=RENAME_FASTA, str=RENAME_STR, renamed=renamed)), fh, indent=0)
    print("wrote %s: %d worlds, %d bytes" % (OUT, len(out), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
