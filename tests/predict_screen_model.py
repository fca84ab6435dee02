"""The rule of the reference's screen_precusor_candidates (utils/screen_precusor_candidates.py, classes/readPrecusor.py)
restated without forgi, for the tests: what mrg_predict_screen_candidates / _prune / _features / _select and
mrg_write_screened_features must give.  Pure Python, no GPU.

The structure elements come from a plain loop model instead of forgi's BulgeGraph:
  * a hairpin is a pair with no pair inside; its element is the unpaired run between the two bases;
  * an interior loop is a loop closed by a pair with exactly one inner pair that is not stacked on it (a one-sided bulge
    counts);
  * a stem is a maximal stack of pairs.
forgi numbers the elements of a kind along the sequence (s0, s1, ...; h0, h1, ...).  The reference's to_element_string
keeps only the LAST CHARACTER of an element's name, so s1 and s11 share the key "s1": adjacent runs of the two merge and
stemLen takes one maximum for both.  element_keys() restates that quirk.

The reference walks elementDic.keys(); the fixtures are captured under Python 3, where that is the order of first
appearance along the sequence, and so is this model's.
"""
import re

PRUNED_LENGTH = 15
CLOSEST, FARTHEST = 9, 44
NONE_ROW = "\t".join(["None"] * 14)
HEADER_TAIL = ("pruned_precusor_seq\tpruned_precusor_str\tarmType\tdistanceToloop\tpercentage_PairedInMiRNA\thairpin_count\t"
               "binding_count\tinteriorLoopCount\tapicalLoop_size\tstem_length\tmFE\tcount_bindings_in_miRNA\tUGU_UGUG_motif\t"
               "pair_state\n")
UPDATED_SUFFIX = "_updated_stableClusterSeq_15.tsv"


class StructureError(ValueError):
    """A structure RNAfold does not write: unbalanced, or a hairpin loop under 3."""


def parse_energy(line):
    """The reference's two-branch parse of the third line of a record: `(-12.30)` / `( -2.30)`; 0.0 where that fails."""
    f = line.strip().split()
    try:
        if len(f[1]) >= 3:
            return float(f[1][1:-1].strip())
        return float(f[2][:-1].strip())
    except (IndexError, ValueError):
        return 0.0


def parse_str(text):
    """[(name, sequence, structure, energy)] of an RNAfold output (three lines a record)."""
    lines = text.splitlines()
    out = []
    for i in range(0, len(lines), 3):
        item = lines[i:i + 3]
        if len(item) < 3:
            raise ValueError("a record of %d lines at line %d" % (len(item), i + 1))
        out.append((item[0].strip()[1:], item[1].strip(), item[2].strip().split()[0], parse_energy(item[2])))
    return out


def pair_table(structure):
    """partner[i] (0-based) or -1; StructureError for brackets that do not balance."""
    pt, stack = [-1] * len(structure), []
    for i, ch in enumerate(structure):
        if ch == "(":
            stack.append(i)
        elif ch == ")":
            if not stack:
                raise StructureError("a `)` without partner at %d" % i)
            j = stack.pop()
            pt[i], pt[j] = j, i
    if stack:
        raise StructureError("a `(` without partner at %d" % stack[-1])
    return pt


def find_pos(mirna, seq):
    s = seq.find(mirna)
    return s, s + len(mirna)


def mirna_structure(mirna, seq, structure):
    s, e = find_pos(mirna, seq)
    return structure[s:e]


def check_arm(seq, structure, mirna):
    ms = mirna_structure(mirna, seq, structure)
    if "(" in ms and ")" in ms and re.search(r"\(.*\)", ms):
        return "loop"
    if "(" in ms:
        return "arm5" if ms.count("(") >= ms.count(")") else "arm3"
    if ")" in ms:
        return "arm3"
    return "unmatchedRegion"


def prune_bounds(seq, structure, mirnas, pruned_length=PRUNED_LENGTH):
    """getPrunedPrecusor up to the fold: the slice (lo, hi) of the sequence, 0 <= lo <= hi <= len, or None where
    pairing_partner returns None.  IndexError where the reference dies of one (the miRNA absent and longer than the sequence by
    two or more)."""
    if len(mirnas) == 1 or find_pos(mirnas[0], seq)[0] == 20:
        sel = mirnas[0]
    else:
        sel = mirnas[1]
    arm = check_arm(seq, structure, sel)
    pt = pair_table(structure)
    s, e = find_pos(sel, seq)
    n = len(seq)
    if arm == "arm5":
        other = 0
        for i in range(s, e):
            if structure[i] == "(":
                break
            other += 1
        q = s + other
        if not 0 <= q < n or pt[q] < 0:
            return None
        cut = slice(s - pruned_length, min(other + pt[q], n - 1) + 1 + pruned_length)
    else:
        other = 0
        for i in range(e - 1, -1, -1):
            if structure[i] == ")":   # (IndexError beyond the structure, as the reference's)
                break
            other += 1
        q = e - other - 1
        if not 0 <= q < n or pt[q] < 0:
            return None
        cut = slice(max(pt[q] - other, 0) - pruned_length, e + pruned_length)
    lo, hi, _ = cut.indices(n)
    return lo, max(lo, hi)


def prune_slice(seq, structure, mirnas, pruned_length=PRUNED_LENGTH):
    """The pruned sequence, or None."""
    cut = prune_bounds(seq, structure, mirnas, pruned_length)
    return None if cut is None else seq[cut[0]:cut[1]]


def elements(structure):
    """(hairpins, interior, stems) of the loop model: hairpins = [(first, last)] of the loops' unpaired runs in sequence
    order, interior = the count, stems = [(i, j, length)] with (i, j) the outermost pair, ordered by i."""
    pt = pair_table(structure)
    n = len(structure)
    hairpins, interior, stems = [], 0, []
    for i in range(n):
        if structure[i] != "(":
            continue
        j = pt[i]
        k = i + 1
        while structure[k] == ".":
            k += 1
        if k == j:
            if j - i - 1 < 3:
                raise StructureError("a hairpin loop of %d at %d" % (j - i - 1, i))
            hairpins.append((i + 1, j - 1))
        else:
            l = pt[k]
            m = l + 1
            while structure[m] == ".":
                m += 1
            if m == j and (k > i + 1 or l < j - 1):
                interior += 1
        if not (i > 0 and structure[i - 1] == "(" and pt[i - 1] == j + 1):
            length = 1
            while structure[i + length] == "(" and pt[i + length] == j - length:
                length += 1
            stems.append((i, j, length))
    return hairpins, interior, stems


def element_keys(structure):
    """The runs of the keys "h<d>" and "s<d>" (d = the last character of the element's number) as the reference's
    elementDic holds them: {key: [[first, last], ...]} in the order of first appearance, from the labels of every position."""
    hairpins, _, stems = elements(structure)
    label = [None] * len(structure)
    for k, (a, b) in enumerate(hairpins):
        for x in range(a, b + 1):
            label[x] = "h" + str(k)[-1]
    for k, (i, j, length) in enumerate(stems):
        for x in range(length):
            label[i + x] = label[j - x] = "s" + str(k)[-1]
    dic, prev = {}, object()
    for x, lab in enumerate(label):
        if lab != prev:
            if lab is not None:
                dic.setdefault(lab, []).append([x, x])
        elif lab is not None:
            dic[lab][-1][1] = x
        prev = lab
    return dic


def _overlap(s, e, region):   # len(set(range(s, e + 1)) & set(range(region[0], region[1] + 1)))
    return max(0, min(e, region[1]) - max(s, region[0]) + 1)


def _arm_entry(seq, structure, mirna, regions):
    arm = check_arm(seq, structure, mirna)
    s, e = find_pos(mirna, seq)
    e -= 1
    over = max([_overlap(s, e, r) for r in regions]) if regions else 0
    if over == 0:
        dist = min([r[0] - 1 - e for r in regions]) if arm == "arm5" else min([s - r[1] - 1 for r in regions])
    else:
        r = next(r for r in regions if _overlap(s, e, r) == over)
        dist = r[0] - 1 - e if arm == "arm5" else s - r[1] - 1
    return arm, [over, dist]


def features(seq, structure, mirnas, mfe):
    """featuresInPrecusor plus percentageOfPairedInMiRNA and bindingsInMiRNA: a dict, or None for the all-None row."""
    if structure is None or "(" not in structure or ")" not in structure:
        return None
    hairpins, interior, stems = elements(structure)
    dic = element_keys(structure)
    regions = [r for key, runs in dic.items() if key[0] == "h" for r in runs]
    arm, entry = _arm_entry(seq, structure, mirnas[0], regions)
    arms = {arm: entry}
    if len(mirnas) == 2:
        arm2, entry2 = _arm_entry(seq, structure, mirnas[1], regions)
        arms[arm2] = entry2
    ms = mirna_structure(mirnas[0], seq, structure)
    bound = ms.count("(") + ms.count(")")
    return dict(hairpin_count=len(hairpins), binding_count=max(structure.count("("), structure.count(")")), interior_count=interior,
                arm=arm, apical=max([r[1] - r[0] + 1 for r in regions]) if regions else 0, arms=arms,
                stem_len=sum(max(r[1] + 1 - r[0] for r in runs) for key, runs in dic.items() if key[0] == "s"),
                ugu="Yes" if any("UGU" in seq[r[0]:r[1]] for r in regions) else "No", mfe=mfe,
                pair_state="Yes" if len(mirnas) == 2 else "No", percent=bound / float(len(ms)) if ms else 0, bindings=bound,
                n_stems=len(stems))


def retained(f, threshold=15):
    """selcteOptimalPrecusor's rule for one candidate's features (not None)."""
    if not (f["hairpin_count"] > 0 and f["binding_count"] >= threshold and f["percent"] >= 0.6):
        return False
    a = f["arms"]
    if "arm5" in a and "arm3" in a:
        return a["arm5"][0] <= 5 and a["arm3"][0] == 0
    if "arm5" in a:
        return a["arm5"][0] <= 5
    if "arm3" in a:
        return a["arm3"][0] == 0
    return False


def select(feature_list, original_mfe):
    """The index of the chosen candidate, or None: the retained ones, otherwise every non-null one; the lowest original
    MFE, ties to the lower index."""
    keep = [i for i, f in enumerate(feature_list) if f is not None and retained(f)]
    if not keep:
        keep = [i for i, f in enumerate(feature_list) if f is not None]
    if not keep:
        return None
    return min(keep, key=lambda i: (original_mfe[i], i))


def read_features(text):
    """(header line, [(line, clusterName, miRNA, neighborState, up, down)]) of a feature file's text."""
    lines = text.splitlines(True)
    if not lines:
        return "", []
    cols = lines[0].strip().split("\t")
    ix = {k: cols.index(k) for k in ("stableClusterSeq", "clusterName", "neighborState", "upstreamDistance", "downstreamDistance")}
    rows = []
    for line in lines[1:]:
        f = line.strip().split("\t")
        dist = [10000 if f[ix[k]] == "None" else int(f[ix[k]]) for k in ("upstreamDistance", "downstreamDistance")]
        rows.append((line, f[ix["clusterName"]], f[ix["stableClusterSeq"]].replace("T", "U"), f[ix["neighborState"]], dist[0], dist[1]))
    return lines[0], rows


def candidates(rows):
    """Per line ([record index in the .str], [[miRNA line, ...] per candidate]); record 2 i is line i's precusor_1, 2 i + 1
    its precusor_2.  IndexError where the reference dies of one."""
    out = []
    n = len(rows)
    for i, (_, name, _, state, up, down) in enumerate(rows):
        near_up, near_down = CLOSEST <= up <= FARTHEST, CLOSEST <= down <= FARTHEST
        if state != "Good":
            out.append(([2 * i, 2 * i + 1], [[i], [i]]))
            continue
        if (near_up and i == 0) or (near_down and i == n - 1) or not (near_up or near_down):
            raise IndexError("line %d (%s): a Good line without the neighbour its distances name" % (i, name))
        if not near_up:
            out.append(([2 * i + 1, 2 * i + 2], [[i, i + 1]] * 2))
        elif near_down:
            out.append(([2 * i - 1, 2 * i, 2 * i + 1, 2 * i + 2], [[i, i - 1]] * 2 + [[i, i + 1]] * 2))
        else:
            out.append(([2 * i - 1, 2 * i], [[i, i - 1]] * 2))
    return out


def format_row(seq, structure, f):
    a = f["arms"][f["arm"]]
    return "%s\t%s\t%s\t%d\t%.2f\t%d\t%d\t%d\t%d\t%d\t%.2f\t%d\t%s\t%s" % (
        seq, structure, f["arm"], a[1], f["percent"], f["hairpin_count"], f["binding_count"], f["interior_count"], f["apical"],
        f["stem_len"], f["mfe"], f["bindings"], f["ugu"], f["pair_state"])


def screen_lines(features_text, str_text, fold, pruned_length=PRUNED_LENGTH, fold_each=False):
    """(header, [per line a dict: line, records, mirnas, original_mfe, candidates = [(pruned, structure, features)], best]).
    fold_each: hand `fold` every candidate's sequence, as the reference folds them, not every distinct one once."""
    header, rows = read_features(features_text)
    records = parse_str(str_text)
    if len(records) != 2 * len(rows):
        raise ValueError("%d records in the .str for %d feature lines" % (len(records), len(rows)))
    cands = candidates(rows)
    pruned = []
    for recs, mirs in cands:
        for r, m in zip(recs, mirs):
            _, seq, structure, _ = records[r]
            pruned.append(prune_slice(seq, structure, [rows[x][2] for x in m], pruned_length))
    todo = [p for p in pruned if p] if fold_each else sorted({p for p in pruned if p})
    folded = dict(zip(todo, fold(todo)))
    out, k = [], 0
    for (line, _, _, _, _, _), (recs, mirs) in zip(rows, cands):
        feats = []
        for r, m in zip(recs, mirs):
            p = pruned[k]
            k += 1
            structure, mfe = folded[p] if p else (None, None)
            feats.append((p, structure, features(p, structure, [rows[x][2] for x in m], mfe) if p else None))
        mfes = [records[r][3] for r in recs]
        out.append(dict(line=line, records=recs, mirnas=mirs, original_mfe=mfes, candidates=feats,
                        best=select([f[2] for f in feats], mfes)))
    return header, out


def screen(features_text, str_text, fold, pruned_length=PRUNED_LENGTH, fold_each=False):
    """The text of `_updated_stableClusterSeq_15.tsv`.  fold(sequences) -> [(structure, energy)], one per sequence."""
    header, lines = screen_lines(features_text, str_text, fold, pruned_length, fold_each)
    out = [header.strip() + "\t" + HEADER_TAIL] if header else []
    for d in lines:
        best = d["best"]
        out.append(d["line"].strip() + "\t" + (NONE_ROW if best is None else format_row(*d["candidates"][best])) + "\n")
    return "".join(out)
