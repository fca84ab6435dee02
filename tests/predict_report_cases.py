"""Inputs for the tests of predict mode's report: worlds of three texts (the novel list, the screened table, the cluster
file) built from hairpins with a consistent geometry -- a cluster at offset a of a precursor that starts at genome position G
pads to exactly the precursor's span on either strand -- and then bent where a case wants it bent; the hand-made inputs on
which the reference raises; and one-line-per-precursor worlds in the shapes the device tests sweep.
tests/golden/make_predict_report_golden.py runs the reference over WORLDS; tests/golden/predict_report.json holds what it gave.
"""
import hashlib
import json
import os
import random

from tests import predict_features_model as features_model
from tests import predict_screen_model as screen_model

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "predict_report.json")
SAMPLE = "smp"
STEM = "unmapped_mirna_%s_vs_representative_seq_modified_selected_sorted" % SAMPLE
TABLE = STEM + "_features_updated_stableClusterSeq_15.tsv"
CLUSTER = STEM + "_cluster.txt"
NOVEL = SAMPLE + "_novel_miRNAs_miRge2.0.csv"
HEADER = (features_model.HEADER_HEAD + features_model.HEADER_TAIL.strip("\n") + "\t" + screen_model.HEADER_TAIL).strip("\n").split("\t")
NOVEL_HEADER = "predictedValue,probability,realMicRNA,realMicRNAName,clusterName\n"
WORLDS = ("hand", "random_a", "random_b", "nothing_listed")
TEXT_WORLDS = ("hand",)     # kept as text in the fixture; the others as SHA-256
# the hand-made world's table: the columns the report reads and a few around them, so that the fixture's text stays small
COMPACT_HEADER = [h for h in HEADER if h in ("realMicRNA", "chr", "clusterName", "clusterSeq", "stableClusterSeq", "alignedClusterSeq", "seqCount",
                                             "readCountSum", "exactMatchRatio", "headUnstableLength", "tailUnstableLength", "neighborState",
                                             "upstreamDistance", "downstreamDistance", "pruned_precusor_seq", "pruned_precusor_str", "armType",
                                             "mFE", "pair_state")]


def golden():
    with open(GOLDEN) as fh:
        return json.load(fh)


def digest(text):
    return hashlib.sha256(text.encode("utf-8")).hexdigest()


CALL_KEYS = ("name", "probability", "chr", "start", "end", "strand", "arm", "mature_reads", "total_reads", "precursor", "structure", "mature",
             "passenger")


def calls_form(calls):
    """The creatPDF calls of a world in one canonical form: the scalars as text and the rows handed over (the mature's, then the
    passenger's) as [padded row, count]; calls_digest is the SHA-256 of its JSON."""
    return [[str(c[k]) for k in CALL_KEYS] + [[[r[0], int(r[1])] for r in c["mature_rows"] + ([] if c["passenger_rows"] == "None" else c["passenger_rows"])]]
            for c in calls]


def calls_digest(form):
    return digest(json.dumps(form, separators=(",", ":")))


def calls_form_from_files(report, profiles):
    """The same form read back from the report and the profile file of a run."""
    lines = report.split("\n")[1:-1]
    blocks = profiles.split(">")[1:]
    assert len(lines) == len(blocks)
    out = []
    for line, block in zip(lines, blocks):
        c, ls = line.split(","), block.split("\n")
        rows = [[t, int(n)] for t, n in (ln.split("\t") for ln in ls[4:-1])]
        total = int(c[9]) + (0 if c[10] == "None" else int(c[10]))
        out.append([c[0], c[1], c[2], c[3], c[4], c[5], c[7], c[9], str(total), c[11], c[12], c[6], c[8], rows])
    return out


def to_dna(rna):
    return rna.replace("U", "T")


def hairpin(rng, stem, loop, flank5, flank3):
    """(RNA, structure) of one stem-loop with unpaired flanks."""
    n = flank5 + 2 * stem + loop + flank3
    return ("".join(rng.choice("ACGU") for _ in range(n)), "." * flank5 + "(" * stem + "." * loop + ")" * stem + "." * flank3)


class World:
    """Lines are added in file order; texts() gives the three files."""

    def __init__(self, header=HEADER):
        self.header, self.rows, self.blocks, self.listed, self.count = list(header), [], [], [], 0

    def line(self, P, S, G, chrom, strand, a, length, hul=0, tul=0, hd=0, td=0, reads=100, up="None", down="None", arm="arm5", pair="Yes",
             prob=None, members=((0, 0, 60), (1, 0, 30), (0, 2, 10)), cluster_seq=None, block=True, own=None):
        """One table line (and its block) for the cluster at P[a : a + length] of a precursor whose first base lies at G (strand +)
        or whose last base lies at G (strand -).  own = (sequence, structure) the line itself carries instead of P, S.
        members: (dashes in front, dashes behind, count) inside the block's width, hd / td dashes wider than the cluster."""
        self.count += 1
        L = len(P)
        cs = to_dna(P[a:a + length]) if cluster_seq is None else cluster_seq
        start = G + a if strand == "+" else G + L - a - length
        end = start + length - 1
        name = "%s:miRCluster_%d_%d:%s:%d_%d%s" % (SAMPLE, self.count, length, chrom, start, end, strand)
        row = dict.fromkeys(HEADER, "0")
        seq, structure = (P, S) if own is None else own
        row.update(realMicRNA="Null", realMicRNAName="Null", chr=chrom, startPos=str(start), endPos=str(end), clusterName=name, clusterSeq=cs,
                   majoritySeq=cs, stableClusterSeq=to_dna(P[a + hul:a + length - tul]), alignedClusterSeq="-" * hd + cs + "-" * td,
                   adjustedClusterSeq=cs, clusterSecondSeq=cs, templateSeq=cs, seqCount=str(len(members)), readCountSum=str(reads),
                   exactMatchRatio="1.0", headUnstableLength=str(hul), tailUnstableLength=str(tul), neighborState="Good",
                   upstreamDistance=str(up), downstreamDistance=str(down), pruned_precusor_seq=seq, pruned_precusor_str=structure, armType=arm,
                   pair_state=pair, UGU_UGUG_motif="No")
        self.rows.append(row)
        if block:
            cl = "-" * hd + cs + "-" * td
            text = ["Cluster Name: %s" % name, "%s (%d - %d%s) cluster %d:" % (chrom, start, end, strand, self.count), cl + ": 1.0",
                    cl + ": 1.0", cl]
            for x, y, count in members:
                text.append("-" * x + cl[x:len(cl) - y].replace("-", "A") + "-" * y + "\t%d" % count)
            self.blocks.append("\n".join(text) + "\n")
        if prob is not None:
            self.listed.append((prob, name))
        return name

    def texts(self, order=None, repeat=()):
        listed = sorted(self.listed, key=lambda pn: -float(pn[0])) if order is None else order
        listed = list(listed) + [(p, listed[k][1]) for k, p in repeat]
        novel = NOVEL_HEADER + "".join("1,%s,Null,Null,%s\n" % pn for pn in listed)
        table = "\t".join(self.header) + "\n" + "".join("\t".join(r[h] for h in self.header) + "\n" for r in self.rows)
        return novel, table, "".join(self.blocks)


def hand_world():
    """Every case the fixture must hold, one unit each (tests/golden/make_predict_report_golden.py: WANTED)."""
    rng = random.Random(5)
    w = World(COMPACT_HEADER)
    # the first data line offers to the header; a negative pad and a ragged row (a member two bases in front of the precursor)
    P, S = hairpin(rng, 24, 8, 4, 6)
    w.line(P, S, 1000, "chr1", "+", 0, 22, hd=2, up=5, prob="0.99", members=((0, 0, 50), (2, 0, 7)))
    # a plain pair: the second offers upstream, both listed, the first has more reads
    P, S = hairpin(rng, 25, 9, 5, 5)
    w.line(P, S, 5000, "chr1", "+", 4, 22, hul=1, tul=2, down=30, prob="0.98", reads=100)
    w.line(P, S, 5000, "chr1", "+", 41, 22, up=30, down=300, prob="0.97", reads=40, arm="arm3")
    # strand -: the first offers downstream its own precursor; only the first is listed
    P, S = hairpin(rng, 26, 7, 6, 6)
    w.line(P, S, 9000, "chr2", "-", 5, 22, up=60, down=20, prob="0.96", reads=70)
    w.line(P, S, 9000, "chr2", "-", 42, 21, up=20, down=200, arm="arm3", reads=90, own=(P[1:-2], S[1:-2]))
    # both neighbours offer to the line between them: the later one's stands; only the second of that pair is listed
    P, S = hairpin(rng, 27, 8, 6, 7)
    w.line(P, S, 15000, "chr3", "+", 3, 22, up=70, down=10, prob="0.95", own=(P + "AC", S + ".."))
    w.line(P, S, 15000, "chr3", "+", 44, 22, up=10, down=12, arm="arm3", reads=300, own=("GG" + P, ".." + S))
    w.line(P, S, 15000, "chr3", "+", 8, 22, up=12, down=400, prob="0.94", reads=20)
    # re-typed to loop (a listed mature that gets no number), and a line that is loop already
    P, S = hairpin(rng, 20, 6, 8, 8)
    w.line(P, S, 20000, "chr4", "+", 20, 24, prob="0.93", pair="No")
    w.line(P + "A", S + ".", 21000, "chr4", "+", 21, 22, arm="loop", pair="No")
    # a clusterSeq that the precursor does not hold (the -1 slice): its first base differs, the stable part starts behind it
    P, S = hairpin(rng, 22, 8, 5, 5)
    cs = to_dna(P[6:28])
    w.line(P, S, 30000, "chr5", "-", 6, 22, hul=1, prob="0.92", pair="No", cluster_seq=("A" if cs[0] != "A" else "C") + cs[1:])
    # a stretch with `)` before `(` only: two hairpins, the cluster over the gap between them
    P1, S1 = hairpin(rng, 12, 5, 2, 2)
    P2, S2 = hairpin(rng, 12, 5, 2, 2)
    w.line(P1 + P2, S1 + S2, 40000, "chr5", "+", 22, 22, prob="0.91", pair="No", arm="arm3")
    # groups of 5, 4 and 3 members (pair_state No: no offers)
    P, S = hairpin(rng, 30, 8, 10, 10)
    for k, (prob, reads, arm) in enumerate([("0.90", 50, "arm5"), ("0.89", 50, "arm5"), (None, 500, "arm5"), ("0.88", 5, "arm3"),
                                             ("0.87", 9, "arm3")]):   # a tie; only the second listed; a single
        w.line(P, S, 50000, "chr6", "+", 2 + 3 * k if k < 3 else 48 + 3 * k, 20, prob=prob, reads=reads, arm=arm, pair="No")
    P, S = hairpin(rng, 30, 8, 10, 10)
    for k, (prob, reads, arm) in enumerate([("0.86", 10, "arm5"), (None, 10, "arm3"), ("0.85", 10, "arm5"), ("0.84", 11, "arm3")]):
        w.line(P, S, 60000, "chr6", "-", 2 + 3 * k if k % 2 == 0 else 50 + k, 20, prob=prob, reads=reads, arm=arm, pair="No")
    P, S = hairpin(rng, 30, 8, 10, 10)
    for k, (prob, reads, arm) in enumerate([("0.83", 10, "arm5"), (None, 99, "loop"), ("0.82", 10, "arm3")]):   # a passenger dropped for loop
        w.line(P, S, 70000, "chr7", "+", (3, 30, 55)[k], 20, prob=prob, reads=reads, arm=arm, pair="No")
    # lines without a precursor, and one nobody lists
    w.line("None", "None", 80000, "chr8", "+", 0, 4, cluster_seq="ACGTTGCATGCATGCAAGTC", arm="None", pair="None", block=False)
    P, S = hairpin(rng, 22, 8, 5, 5)
    w.line(P, S, 90000, "chr8", "-", 5, 22, pair="No")
    return w.texts(repeat=((1, "0.5"),))   # the second name once more at the end of the list


def random_world(seed, units=60):
    rng = random.Random(seed)
    w = World()
    G = 1000
    for _ in range(units):
        G += rng.randrange(500, 5000)
        chrom, strand = "chr%d" % rng.randrange(1, 4), rng.choice("+-")
        P, S = hairpin(rng, rng.randrange(24, 34), rng.randrange(4, 12), rng.randrange(4, 10), rng.randrange(4, 10))
        L = len(P)
        members = lambda: tuple((rng.randrange(0, 3), rng.randrange(0, 3), rng.randrange(1, 10 ** rng.randrange(1, 7))) for _ in range(rng.randrange(1, 9)))
        prob = lambda: "%.6f" % rng.uniform(0.8, 1.0) if rng.random() < 0.7 else None
        kind = rng.random()
        if kind < 0.3:   # a single; now and then over the loop
            a = rng.randrange(3, L - 26) if rng.random() < 0.7 else S.index("(") + 8
            w.line(P, S, G, chrom, strand, a, 22, hul=rng.randrange(0, 3), tul=rng.randrange(0, 3), prob="%.6f" % rng.uniform(0.8, 1.0),
                   pair="No", members=members(), reads=rng.randrange(10, 1000), hd=rng.randrange(0, 2), td=rng.randrange(0, 2))
        elif kind < 0.8:   # a pair; the second one's precursor now and then shorter at both ends
            d = rng.randrange(10, 60)
            pa, pb = prob(), prob()
            t1, t2 = (rng.randrange(0, 3), rng.randrange(0, 3)) if rng.random() < 0.5 else (0, 0)
            a, b = rng.randrange(3, 7), L - 22 - rng.randrange(3, 7)
            w.line(P, S, G, chrom, strand, a, 22, hul=rng.randrange(0, 2), up=rng.choice(("None", 60, 90)), down=d, prob=pa, members=members(),
                   reads=rng.randrange(10, 400))
            w.line(P, S, G, chrom, strand, b, 22, tul=rng.randrange(0, 2), up=d, down=100, prob=pb, arm="arm3", members=members(),
                   reads=rng.randrange(10, 400), own=(P[t1:L - t2], S[t1:L - t2]))
        else:   # a group of 3 to 5 on one precursor: every member listed
            for k in range(rng.randrange(3, 6)):
                w.line(P, S, G, chrom, strand, 3 + 4 * k, 21, prob="%.6f" % rng.uniform(0.8, 1.0), pair="No", arm=rng.choice(("arm5", "arm3", "loop")),
                       members=members(), reads=rng.randrange(10, 50))
    return w.texts()


def nothing_listed_world():
    novel, table, cluster = random_world(3, units=6)
    return NOVEL_HEADER, table, cluster


def world(name):
    if name == "hand":
        return hand_world()
    if name == "random_a":
        return random_world(20261021)
    if name == "random_b":
        return random_world(77, units=90)
    if name == "nothing_listed":
        return nothing_listed_world()
    raise KeyError(name)


def timing_world(lines=10000, listed=2000, seed=1):
    """About `lines` table lines of which about `listed` are in the novel list (scripts/predict_report_timing.py)."""
    rng = random.Random(seed)
    w = World()
    G = 1000
    share = listed / float(lines)
    while len(w.rows) < lines:
        G += 3000
        P, S = hairpin(rng, 28, 8, 6, 6)
        members = tuple((rng.randrange(0, 3), rng.randrange(0, 3), rng.randrange(1, 5000)) for _ in range(rng.randrange(2, 12)))
        pa = "%.6f" % rng.uniform(0.8, 1.0) if rng.random() < share else None
        pb = "%.6f" % rng.uniform(0.8, 1.0) if rng.random() < share else None
        w.line(P, S, G, "chr%d" % rng.randrange(1, 20), "+-"[len(w.rows) % 4 == 0], 5, 22, down=30, prob=pa, members=members)
        w.line(P, S, G, w.rows[-1]["chr"], w.rows[-1]["clusterName"][-1], 40, 22, up=30, down=100, prob=pb, arm="arm3", members=members)
    return w.texts()


# ------------------------------------------------------------------------------------------------ where the reference raises
def raising_cases():
    """name -> the three texts; on each the reference raises and the stage raises ValueError."""
    rng = random.Random(9)
    out = {}
    P, S = hairpin(rng, 25, 8, 5, 5)
    w = World()   # the last line offers downstream
    w.line(P, S, 1000, "chr1", "+", 4, 22, prob="0.9", pair="No")
    w.line(P, S, 5000, "chr1", "+", 4, 22, up=60, down=20, prob="0.95")
    out["last_line_offers_downstream"] = w.texts()
    w = World()   # int('None')
    w.line(P, S, 1000, "chr1", "+", 4, 22, up=60, down="None", prob="0.9")
    w.line(P, S, 5000, "chr1", "+", 4, 22, prob="0.95", pair="No")
    out["downstream_none_behind_a_far_upstream"] = w.texts()
    w = World()   # a listed name without a precursor
    w.line("None", "None", 1000, "chr1", "+", 0, 4, cluster_seq="ACGTACGTACGTACGTACGT", prob="0.9", arm="None", pair="None")
    out["listed_without_precursor"] = w.texts()
    w = World()   # a group of four: the second pair has no listed member, and its chosen mature is arm3
    for k, prob in enumerate(("0.9", None, None, None)):
        w.line(P, S, 1000, "chr1", "+", 3 + 4 * k, 22, prob=prob, pair="No", arm="arm3")
    out["pair_without_a_listed_member"] = w.texts()
    w = World()   # the stable sequence is not in the precursor the neighbour hands over
    Q, T = hairpin(rng, 25, 8, 5, 5)
    w.line(P, S, 1000, "chr1", "+", 4, 22, down=30, prob="0.9")
    w.line(Q, T, 1000, "chr1", "+", 40, 22, up=30, down=100, prob="0.95", arm="arm3")
    out["stable_sequence_absent"] = w.texts()
    return out


# ------------------------------------------------------------------------------------------------ the device tests' shapes
def shape_world(n_lines, prec_len=80, placement="middle", n_rows=3, count=10, seed=0, cs_len=22):
    """n_lines single-line precursors of prec_len characters, every line listed: the clusterSeq at offset 0 (`first`), at the
    last possible offset (`last`), across position 64 (`straddle`), absent (`absent`: stable part one base shorter) or longer
    than the precursor (`longer`).  Every block holds n_rows rows of `count` reads."""
    rng = random.Random(seed * 1000 + n_lines + prec_len)
    w = World()
    for k in range(n_lines):
        L = prec_len
        P = "".join(rng.choice("ACGU") for _ in range(L))
        half = max((L - 3) // 2, 0)
        S = ("(" * half + "." * (L - 2 * half) + ")" * half)[:L] if k % 2 else "." * L   # (every other line: re-typed where it spans the loop)
        n = min(cs_len, L)
        a = {"first": 0, "last": L - n, "middle": (L - n) // 2, "straddle": max(min(64 - n // 2, L - n), 0), "absent": 0, "longer": 0}[placement]
        kw = {}
        if placement == "absent" and n > 1:
            cs = to_dna(P[a:a + n])
            kw = dict(hul=1, cluster_seq=("A" if cs[0] != "A" else "C") + cs[1:])
        if placement == "longer":
            n, kw = L, dict(tul=0, cluster_seq=to_dna(P) + "ACGT")
        members = tuple((i % 3 if n > 4 else 0, (i // 3) % 2 if n > 4 else 0, count + i) for i in range(n_rows))
        w.line(P, S, 1000 + 1000 * k, "chr%d" % (1 + k % 3), "+-"[k % 2], a, n, prob="0.%d" % (99999 - k), pair="No", arm="arm5" if k % 3 else "arm3",
               members=members, **kw)
    return w.texts()
