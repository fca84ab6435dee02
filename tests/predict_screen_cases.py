"""What tests/predict_screen_model.py gives, laid out as the mrg_predict_screen_* calls take and leave it: blobs (offsets plus
bytes), candidate slots, status bytes and 16-word feature rows; and the inputs of the fixture's direct calls, which the fixture
does not repeat: case_inputs() makes them from a generator of its own (no `random`: the same list under every Python), the
fixture holds their SHA-256 and the reference's results.  Shared by the maker, the CPU and the GPU tests; Python and numpy."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

from tests import predict_features_model as features_model
from tests import predict_precursors_model as precursors_model
from tests import predict_screen_model as model

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "predict_screen.json")
STANDIN = os.path.join(HERE, "fold_standin.py")
NO = 0xffffffff
ARMS = ("loop", "arm5", "arm3", "unmatchedRegion")
WORDS = ("state", "hairpins", "bindings", "interior", "arm1", "apical", "over1", "dist1", "arm2", "over2", "dist2", "stem_len", "ugu",
         "bound", "mir_len", "stems")
PRECURSORS = os.path.join(HERE, "golden", "predict_precursors.json")
HEADER = features_model.HEADER_HEAD + features_model.HEADER_TAIL
COLUMNS = HEADER.rstrip("\n").split("\t")
N_CASES = 1500
_golden = {}


class Lcg:
    """The few draws the case generator needs, from a 64-bit linear congruential generator."""

    def __init__(self, seed):
        self.x = seed

    def below(self, n):
        self.x = (self.x * 6364136223846793005 + 1442695040888963407) % (1 << 64)
        return (self.x >> 33) % n

    def random(self):
        return self.below(1 << 20) / float(1 << 20)

    def randint(self, a, b):
        return a + self.below(b - a + 1)

    def choice(self, items):
        return items[self.below(len(items))]


def random_structure(rng, n):
    """A balanced structure of length n with hairpin loops of 3 or more."""
    def inner(n, depth):
        if n < 5 or (depth and rng.random() < 0.25):
            return "." * n
        choice = rng.random()
        if choice < 0.45:       # a pair around the rest, dots outside
            left = rng.randint(0, min(3, n - 5))
            right = rng.randint(0, min(3, n - 5 - left))
            return "." * left + "(" + inner(n - 2 - left - right, depth + 1) + ")" + "." * right
        if choice < 0.75 and n >= 10:
            cut = rng.randint(5, n - 5)
            return inner(cut, depth) + inner(n - cut, depth)
        return "." + inner(n - 1, depth)
    while True:
        s = inner(n, 0)
        if "()" not in s and "(.)" not in s and "(..)" not in s:   # (no hairpin loop RNAfold does not write)
            return s


def units(kind, count):
    """`count` stems (kind "s": one hairpin in count - 1 bulged pairs) or hairpins (kind "h") in the fewest bases."""
    if kind == "h":
        return "(...)" * count
    out = "(...)"
    for _ in range(count - 1):
        out = "(." + out + ")"
    return out


def case_inputs():
    """[(sequence, structure, [miRNA1(, miRNA2)])] of the fixture's N_CASES direct calls: hand-made ones, 9 .. 11 stems and
    hairpins, lengths 63 .. 257, then random short ones."""
    if "inputs" in _golden:
        return _golden["inputs"]
    rng = Lcg(20240607)
    rna = lambda n: "".join(rng.choice("ACGU") for _ in range(n))
    sub = lambda seq, lo, n: seq[lo:lo + n]
    out = []
    s = "(((((....)))))..(((((....)))))"
    q = rna(len(s))
    out.append((q, s, [q[12:18]]))                                       # between two hairpins: overlap 0
    out.append((q, s, [q[4:26]]))                                        # covers both loops whole: equal overlap
    q2 = q[:6] + "AUGU" + q[10:]
    out.append((q2, s, [q2[0:5]]))                                       # UGU ends on the loop's last base
    q3 = q[:5] + "UGUA" + q[9:]
    out.append((q3, s, [q3[0:5]]))                                       # UGU inside
    out += [("A", ".", ["A"]), ("A", ".", ["C"]), (rna(30), "." * 30, ["ACG"])]
    for count, kind in ((10, "s"), (11, "s"), (10, "h"), (9, "s"), (9, "h"), (11, "h")):
        s = units(kind, count)
        q = rna(len(s))
        out += [(q, s, [sub(q, lo, 8)]) for lo in (0, len(s) // 3, len(s) // 2)]
    for n in (63, 64, 65, 255, 256, 257):
        for _ in range(4):
            s, q = random_structure(rng, n), rna(n)
            out.append((q, s, [sub(q, rng.randint(0, n - 22), 22)]))
            out.append((q, s, [sub(q, 20, 20), sub(q, rng.randint(0, n - 22), 22)]))
    while len(out) < N_CASES:
        n = rng.choice([5, 8, 12, 20, 24, 30, 36, 40, 48, 56])
        s, q = random_structure(rng, n), rna(n)
        m = rng.randint(1, min(22, n))
        kind = rng.random()
        if kind < 0.12:
            mirnas = [rna(rng.randint(1, min(6, n + 1)))]                # mostly absent
        elif kind < 0.7:
            mirnas = [sub(q, rng.randint(0, n - m), m)]
        elif n > 24:
            mirnas = [sub(q, rng.choice([20, 20, rng.randint(0, n - 4)]), 4), sub(q, rng.randint(0, n - m), m)]
        else:
            mirnas = [sub(q, rng.randint(0, n - m), m), sub(q, rng.randint(0, n - m), m)]
        out.append((q, s, mirnas))
    _golden["inputs"] = out
    return out


COMPLEMENT = str.maketrans("ACGT", "TGCA")


def revcomp(s):
    return s.translate(COMPLEMENT)[::-1]


def feature_line(ch, start, end, seq, state, up, down, number):
    f = ["."] * len(COLUMNS)
    f[5] = "smp:miRCluster_%d_%d:%s:%d_%d+" % (number, end - start + 1, ch, start, end)
    for k in ("stableClusterSeq", "alignedClusterSeq"):
        f[COLUMNS.index(k)] = seq
    f[COLUMNS.index("headUnstableLength")] = f[COLUMNS.index("tailUnstableLength")] = "0"
    f[COLUMNS.index("neighborState")] = state
    f[COLUMNS.index("upstreamDistance")] = "None" if up is None else str(up)
    f[COLUMNS.index("downstreamDistance")] = "None" if down is None else str(down)
    return "\t".join(f) + "\n"


def hand_world(seed=0):
    """(feature file text, `_features_precusor.fa` text) of the world `screen_hand`.  One `+` chromosome: units of hairpins 150 nt apart, every unit's clusters in file order.  The clusters' distances are
    those between their intervals, as the feature stage would print them."""
    rng = Lcg(seed)
    dna = lambda n: "".join(rng.choice("ACGT") for _ in range(n))
    chrom, lines, number = [dna(150)], [], [0]

    def unit(parts, state):
        """parts: strings, or (string,) for a cluster; consecutive clusters of a unit are neighbours."""
        pos, found = sum(len(c) for c in chrom), []
        for p in parts:
            text = p[0] if isinstance(p, tuple) else p
            if isinstance(p, tuple):
                found.append((pos + 1, pos + len(text), text))
            chrom.append(text)
            pos += len(text)
        chrom.append(dna(150))
        for k, (s, e, text) in enumerate(found):
            number[0] += 1
            up = found[k][0] - found[k - 1][1] - 1 if k else None
            down = found[k + 1][0] - e - 1 if k + 1 < len(found) else None
            lines.append(feature_line("chr1", s, e, text, state, up, down, number[0]))
    a = dna(22)
    unit([(a,), dna(9), revcomp(a)], "Null")                               # a 5' arm alone
    a = dna(22)
    unit([revcomp(a), dna(9), (a,)], "Bad")                                # a 3' arm alone
    a = dna(22)
    unit([(a,), dna(12), (revcomp(a),)], "Good")                           # both arms: branches 1 and 3
    a, b = dna(22), dna(22)
    unit([(a,), dna(10), (revcomp(a)[:11] + revcomp(b)[11:],), dna(10), (b,)], "Good")   # three in a row: branch 2 in the middle
    a, b = dna(22), dna(22)
    unit([(a,), dna(11), (revcomp(a),), dna(30), (b,), dna(11), (revcomp(b),)], "Good")
    unit(["A" * 120, ("A" * 22,), "A" * 120], "Null")                      # nothing pairs: every candidate is null
    a = dna(21)
    unit([(a,), dna(5), revcomp(a)], "Null")
    text = "".join(lines)
    text = text[:-1] + " \t\n"                                             # (trailing whitespace on the last line: line.strip())
    features = HEADER + text
    return features, precursors_model.run(features, {"chr1": "".join(chrom)})


def text_digest(text):
    return hashlib.sha256(text.encode("ascii")).hexdigest()


def str_of(fasta, folds):
    """The `.str` of a FASTA: every record's two lines, then its fold (structure and energy)."""
    lines = fasta.splitlines(True)
    return "".join(lines[2 * k] + lines[2 * k + 1] + fold + "\n" for k, fold in enumerate(folds))


def inputs_digest(inputs):
    return text_digest("\n".join("%s %s %s" % (q, s, ",".join(m)) for q, s, m in inputs))


def pack_case(seq, mirnas, pruned, feat):
    """The reference's results for one call as a short list of numbers: [lo, hi] of the pruned slice ([-1] for None),
    then, unless featuresInPrecusor gave the all-None tuple, hairpinCount, bindingCount, interiorLoopCount, the arm, the
    apical loop, stemLen, the UGU flag, percentageOfPairedInMiRNA as bindingsInMiRNA over the length it was divided by (0: the
    reference's `except`), and armTypeOverlenDic: (overlap, distance) for one miRNA, else (arm, overlap, distance) per arm.  pairState is left out: it says whether
    there are two miRNAs, and the maker asserts that."""
    lo = seq.find(pruned) if pruned else 0
    row = [-1] if pruned is None else [lo, lo + len(pruned)]
    if feat is None:
        return row
    hairpins, bindings, interior, arm, apical, arms, stem_len, ugu, _, pair_state, percent, bound = feat
    length = int(round(bound / percent)) if percent else 0
    assert pair_state == ("Yes" if len(mirnas) == 2 else "No")
    row += [hairpins, bindings, interior, ARMS.index(arm), apical, stem_len, int(ugu == "Yes"), bound, length]
    if len(mirnas) == 1:
        return row + arms[arm]
    for key, (over, dist) in arms.items():
        row += [ARMS.index(key), over, dist]
    return row


def unpack_case(seq, mirnas, row, mfe=-1.5):
    """(pruned, feat) in the reference's own shapes."""
    pruned = None if row[0] < 0 else seq[row[0]:row[1]]
    row = [-1] + row if row[0] < 0 else row
    if len(row) == 2:
        return pruned, None
    hairpins, bindings, interior, arm, apical, stem_len, ugu, bound, length = row[2:11]
    arms = {ARMS[arm]: row[11:13]} if len(mirnas) == 1 else {ARMS[row[k]]: [row[k + 1], row[k + 2]] for k in range(11, len(row), 3)}
    return pruned, [hairpins, bindings, interior, ARMS[arm], apical, arms, stem_len, "Yes" if ugu else "No", mfe, "Yes" if len(mirnas) == 2 else "No",
                    bound / float(length) if length else 0, bound]


def golden():
    """The fixture as the tests read it: "cases" = [[sequence, structure, miRNAs, pruned, features]] in the reference's own
    shapes, "worlds" = [dict(name, features, precursors, str, table, holds)]."""
    if "golden" in _golden:
        return _golden["golden"]
    with open(GOLDEN) as fh:
        raw = json.load(fh)
    inputs = case_inputs()
    assert inputs_digest(inputs) == raw["inputs_sha256"], "case_inputs() no longer makes the calls the fixture was captured for"
    cases = [[q, s, m] + list(unpack_case(q, m, row)) for (q, s, m), row in zip(inputs, raw["cases"])]
    with open(PRECURSORS) as fh:
        shared = {w["name"]: w for w in json.load(fh)["worlds"]}
    worlds = []
    for w in raw["worlds"]:
        src = shared[w["name"]] if w["name"] in shared else dict(zip(("features", "precursors"), hand_world()))
        assert text_digest(src["features"] + src["precursors"]) == w["sha256"], "%s: not the texts the fixture was captured for" % w["name"]
        lines = src["features"].splitlines(True)
        table = "".join([lines[0].strip() + "\t" + model.HEADER_TAIL] + [line.strip() + "\t" + tail + "\n" for line, tail in zip(lines[1:], w["tails"])])
        worlds.append(dict(name=w["name"], features=src["features"], precursors=src["precursors"], str=str_of(src["precursors"], w["folds"]),
                           table=table, holds=w["holds"]))
    _golden["golden"] = dict(cases=cases, worlds=worlds)
    return _golden["golden"]


def blob(strings):
    """(offsets uint64 [n + 1], bytes) of a list of str."""
    off = np.zeros(len(strings) + 1, np.uint64)
    if strings:
        off[1:] = np.cumsum([len(s) for s in strings])
    return off, "".join(strings).encode("ascii")


def row_of(seq, structure, mirnas):
    """The 16 words mrg_predict_screen_features leaves for a candidate within the kernels' limits, by the model; state 2
    (the rest undefined) where the kernels leave it to the host."""
    row = [0] * 16
    row[8] = -1
    f = model.features(seq, structure, mirnas, 0.0)
    if f is None:
        return row
    hairpins, _, stems = model.elements(structure)
    arms = []
    for m in mirnas:
        regions = [r for key, runs in model.element_keys(structure).items() if key[0] == "h" for r in runs]
        arms.append(model._arm_entry(seq, structure, m, regions))
    ms = model.mirna_structure(mirnas[0], seq, structure)
    row = [1, len(hairpins), f["binding_count"], f["interior_count"], ARMS.index(arms[0][0]), f["apical"], arms[0][1][0], arms[0][1][1],
           -1, 0, 0, f["stem_len"], int(f["ugu"] == "Yes"), f["bindings"], len(ms), len(stems)]
    if len(mirnas) == 2:
        row[8:11] = [ARMS.index(arms[1][0]), arms[1][1][0], arms[1][1][1]]
    if len(seq) > 256 or len(stems) >= 10 or len(hairpins) >= 10:
        row[0] = 2
    return row


def takes_host_path(seq, structure):
    if len(seq) > 256:
        return True
    if "(" not in structure:
        return False
    hairpins, _, stems = model.elements(structure)
    return len(stems) >= 10 or len(hairpins) >= 10


def prune_expected(seq, structure, mirnas):
    """(status, lo, hi) mrg_predict_screen_prune leaves: 2 beyond 256 characters."""
    if len(seq) > 256 or any(len(m) > 255 for m in mirnas):
        return 2, 0, 0
    cut = model.prune_bounds(seq, structure, mirnas)
    return (0, 0, 0) if cut is None else (1,) + cut


def fold_many(seqs):
    """[(structure, energy)] of the stand-in folder, one process for all."""
    text = "".join(">c%d\n%s\n" % (k, s) for k, s in enumerate(seqs))
    out = subprocess.run([sys.executable, STANDIN, "--noPS", "--noLP"], input=text, capture_output=True, text=True, check=True).stdout
    return [(r[2], r[3]) for r in model.parse_str(out)]


_world_arrays = {}


def world_arrays(w):
    """The arrays of a golden world by the model (folded once per world and kept): n lines, cand_n, cand_rec [4 n], cand_mir
    [4 n, 2], the records' and the miRNAs' blobs, status, lo, hi [4 n], the pruned blob with its structures and energies,
    feat [4 n, 16] and best [n]."""
    if w["name"] in _world_arrays:
        return _world_arrays[w["name"]]
    _, rows = model.read_features(w["features"])
    records = model.parse_str(w["str"])
    _, lines = model.screen_lines(w["features"], w["str"], fold_many)
    n = len(rows)
    cand_n = np.zeros(n, np.uint8)
    cand_rec, cand_mir = np.full(4 * n, NO, np.uint32), np.full((4 * n, 2), NO, np.uint32)
    status, lo, hi = np.full(4 * n, 3, np.uint8), np.zeros(4 * n, np.uint32), np.zeros(4 * n, np.uint32)
    pruned, structures, p_mfe = [""] * (4 * n), [""] * (4 * n), np.zeros(4 * n)
    feat = np.zeros((4 * n, 16), np.int32)
    feat[:, 8] = -1
    best = np.full(n, -1, np.int32)
    for i, d in enumerate(lines):
        cand_n[i] = len(d["records"])
        best[i] = -1 if d["best"] is None else d["best"]
        for k, (r, m, (p, structure, f)) in enumerate(zip(d["records"], d["mirnas"], d["candidates"])):
            c = 4 * i + k
            cand_rec[c] = r
            cand_mir[c, :len(m)] = m
            mirnas = [rows[x][2] for x in m]
            status[c], lo[c], hi[c] = prune_expected(records[r][1], records[r][2], mirnas)
            if p:
                pruned[c], structures[c], p_mfe[c] = p, structure, f["mfe"] if f else 0.0
                feat[c] = row_of(p, structure, mirnas)
    rec_off, rec_seq = blob([r[1] for r in records])
    mir_off, mir = blob([r[2] for r in rows])
    p_off, p_seq = blob(pruned)
    out = dict(n=n, cand_n=cand_n, cand_rec=cand_rec, cand_mir=cand_mir, rec_off=rec_off, rec_seq=rec_seq,
               rec_str=blob([r[2] for r in records])[1], rec_mfe=np.array([r[3] for r in records], np.float64), mir_off=mir_off, mir=mir,
               status=status, lo=lo, hi=hi, p_off=p_off, p_seq=p_seq, p_str=blob(structures)[1], p_mfe=p_mfe, feat=feat, best=best,
               states=[r[3] for r in rows], up=[r[4] for r in rows], down=[r[5] for r in rows])
    _world_arrays[w["name"]] = out
    return out


def fold_file(fasta_path, str_path):
    """The `fold` callable of predict.screen_precursors over the stand-in."""
    with open(fasta_path, "rb") as src, open(str_path, "wb") as dst:
        subprocess.run([sys.executable, STANDIN, "--noPS", "--noLP"], stdin=src, stdout=dst, check=True)
