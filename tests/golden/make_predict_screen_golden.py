#!/usr/bin/env python3
"""Capture tests/golden/predict_screen.json from the REFERENCE's own utils/screen_precusor_candidates.py,
classes/readPrecusor.py and its forgi copy.

    python tests/golden/make_predict_screen_golden.py <reference src/mirge directory>

Run only in the build container: the modules are copied to a scratch directory outside the repository, CRLF stripped,
converted with lib2to3 and imported from there next to stand-ins for Bio.Seq and Bio.Alphabet (which this script writes
into that directory) and one shim, itertools.izip = zip.  The fold command handed to the reference is
tests/fold_standin.py.  Only data is written into the repository:

  worlds  per world the third line of every record of the `.str` (structure and energy: the stand-in's fold of
          `_features_precusor.fa`) and the 14 columns the reference's `_updated_stableClusterSeq_15.tsv` adds to every line,
          with the SHA-256 of the two input texts.  The texts themselves are not repeated: `main`, `mapped` and the header-only
          `hand_empty` are predict_precursors.json's, `screen_hand` is tests/predict_screen_cases.hand_world(), a chromosome
          of hairpins; WANTED names what it must hold and main() asserts every case.
  cases   the reference's results for the direct calls tests/predict_screen_cases.case_inputs() lists (the fixture holds that
          list's SHA-256, not the list): the first element of getPrunedPrecusor's triple as a slice of the sequence, and
          featuresInPrecusor's tuple with percentageOfPairedInMiRNA and bindingsInMiRNA as numbers (cases.pack_case; main()
          asserts that unpack_case gives the reference's values back).  CASE_WANTED names what the calls must cover; main()
          asserts that list too.
"""
import importlib
import itertools
import json
import os
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import predict_screen_cases as cases  # noqa: E402
from tests import predict_screen_model as model  # noqa: E402

OUT = os.path.join(HERE, "predict_screen.json")
PRECURSORS = os.path.join(HERE, "predict_precursors.json")
STANDIN = os.path.join(os.path.dirname(HERE), "fold_standin.py")
TABLE = "unmapped_mirna_smp_vs_representative_seq_modified_selected_sorted_features.tsv"
STANDINS = {
    "Bio/__init__.py": "",
    "Bio/Alphabet/__init__.py": "generic_dna = None\n",
    "Bio/Seq.py": '''class Seq(object):
    def __init__(self, data, alphabet=None):
        self.data = data

    def transcribe(self):
        return Seq(self.data.replace("T", "U"))

    def __str__(self):
        return self.data
''',
}


def load_reference(src):
    tmp = tempfile.mkdtemp(prefix="predict_screen_golden_")
    for rel, text in STANDINS.items():
        os.makedirs(os.path.dirname(os.path.join(tmp, rel)), exist_ok=True)
        with open(os.path.join(tmp, rel), "w") as fh:
            fh.write(text)
    root = os.path.join(tmp, "mirge")
    shutil.copytree(os.path.join(src, "forgi"), os.path.join(root, "forgi"), ignore=shutil.ignore_patterns("*.pyc", "__pycache__"))
    for sub, name in (("classes", "readPrecusor.py"), ("utils", "screen_precusor_candidates.py")):
        os.makedirs(os.path.join(root, sub))
        shutil.copy(os.path.join(src, sub, name), os.path.join(root, sub, name))
    for d, _, files in os.walk(root):
        if "__init__.py" not in files:
            open(os.path.join(d, "__init__.py"), "w").close()
        for f in files:
            if f.endswith(".py"):
                with open(os.path.join(d, f), "rb") as fh:
                    data = fh.read().replace(b"\r\n", b"\n")
                with open(os.path.join(d, f), "wb") as fh:
                    fh.write(data)
    subprocess.run([sys.executable, "-m", "lib2to3", "-w", "-n", root], capture_output=True, check=True)
    itertools.izip = zip
    sys.path.insert(0, tmp)
    return tmp, importlib.import_module("mirge.classes.readPrecusor"), importlib.import_module("mirge.utils.screen_precusor_candidates")


def fold_texts(fasta_text):
    return subprocess.run([sys.executable, STANDIN, "--noPS", "--noLP"], input=fasta_text, capture_output=True, text=True, check=True).stdout


def fold_many(seqs):
    out = fold_texts("".join(">c%d\n%s\n" % (k, s) for k, s in enumerate(seqs)))
    return [(r[2], r[3]) for r in model.parse_str(out)]


def renamed(fasta_text, str_text):
    names, lines = fasta_text.splitlines(True)[0::2], str_text.splitlines(True)
    return "".join(names[i] + "".join(lines[3 * i + 1:3 * i + 3]) for i in range(len(names)))


def properties(features, str_text):
    got = set()
    _, rows = model.read_features(features)
    _, lines = model.screen_lines(features, str_text, fold_many)
    for (_, _, _, state, up, down), d in zip(rows, lines):
        n = len(d["records"])
        if state != "Good":
            got.add("not_good")
        else:
            near_up, near_down = model.CLOSEST <= up <= model.FARTHEST, model.CLOSEST <= down <= model.FARTHEST
            got.add("good_down_only" if not near_up else "good_both" if near_down else "good_up_only")
        feats = [c[2] for c in d["candidates"]]
        if d["best"] is None:
            got.add("all_null")
            continue
        if n == 4 and d["best"] in (0, 3):
            got.add("four_candidates_neighbour_chosen")
        keep = [i for i, f in enumerate(feats) if f is not None and model.retained(f)]
        pool = keep or [i for i, f in enumerate(feats) if f is not None]
        if sum(d["original_mfe"][i] == d["original_mfe"][d["best"]] for i in pool) > 1:
            got.add("mfe_tie")
        if any(f is None for f in feats):
            got.add("some_null")
        for i in keep:
            arms = feats[i]["arms"]
            got.add("retained_both_arms" if "arm5" in arms and "arm3" in arms else "retained_arm5_only" if "arm5" in arms else "retained_arm3_only")
        if not keep:
            got.add("none_retained")
    return got


WANTED = {"not_good", "good_down_only", "good_both", "good_up_only", "all_null", "four_candidates_neighbour_chosen", "mfe_tie",
          "retained_both_arms", "retained_arm5_only", "retained_arm3_only"}


# ---------------------------------------------------------------------------------------------- the direct cases
def case_properties(seq, structure, mirnas, pruned, feat):
    got = set()
    n = len(seq)
    if n in (1, 63, 64, 65, 255, 256, 257):
        got.add("length_%d" % n)
    if "(" not in structure:
        got.add("no_pairs")
    else:
        hairpins, _, stems = model.elements(structure)
        for count, kind in ((len(stems), "stems"), (len(hairpins), "hairpins")):
            if count in (10, 11):
                got.add("%d_%s" % (count, kind))
        if feat is not None:
            got.add("arm_" + feat["arm"])
            got.add("overlap_positive" if feat["arms"][feat["arm"]][0] > 0 else "overlap_zero")
            s, e = model.find_pos(mirnas[0], seq)
            regions = [r for key, runs in model.element_keys(structure).items() if key[0] == "h" for r in runs]
            over = [model._overlap(s, e - 1, r) for r in regions]
            if max(over) > 0 and over.count(max(over)) > 1:
                got.add("two_hairpins_equal_overlap")
            if any(seq[r[1] - 2:r[1] + 1] == "UGU" and "UGU" not in seq[r[0]:r[1]] for r in regions):
                got.add("ugu_ends_on_last_loop_base")
            if feat["ugu"] == "Yes":
                got.add("ugu_yes")
    s = seq.find(mirnas[0] if len(mirnas) == 1 or seq.find(mirnas[0]) == 20 else mirnas[1])
    if s < 0:
        got.add("mirna_absent")
    elif s < 15:
        got.add("negative_slice_start")
    if pruned is None:
        got.add("partner_none")
    if len(mirnas) == 2:
        got.add("two_mirnas_first_at_20" if seq.find(mirnas[0]) == 20 else "two_mirnas_second_selected")
    return got


CASE_WANTED = {"length_1", "length_63", "length_64", "length_65", "length_255", "length_256", "length_257", "no_pairs", "10_stems",
               "11_stems", "10_hairpins", "arm_loop", "arm_arm5", "arm_arm3", "arm_unmatchedRegion", "overlap_zero",
               "overlap_positive", "two_hairpins_equal_overlap", "ugu_ends_on_last_loop_base", "ugu_yes", "mirna_absent",
               "negative_slice_start", "partner_none", "two_mirnas_first_at_20", "two_mirnas_second_selected"}


def run_case(rp, tmp, seq, structure, mirnas):
    inst = rp.ReadPrecusor("true", "case", seq, structure, -1.5, tmp, 15, *mirnas)
    try:
        pruned = inst.getPrunedPrecusor()[0]
    except Exception as e:   # noqa: BLE001 (the type is the datum)
        pruned = {"error": type(e).__name__}
    try:
        f = inst.featuresInPrecusor()
        feat = None if f[0] is None else list(f) + [inst.percentageOfPairedInMiRNA(), inst.bindingsInMiRNA()]
    except Exception as e:   # noqa: BLE001
        feat = {"error": type(e).__name__}
    return pruned, feat


def model_case(seq, structure, mirnas):
    """The same two results from the model, in the fixture's shape."""
    try:
        pruned = model.prune_slice(seq, structure, mirnas)
    except (IndexError, model.StructureError) as e:
        pruned = {"error": type(e).__name__}
    f = model.features(seq, structure, mirnas, -1.5)
    feat = None if f is None else [f["hairpin_count"], f["binding_count"], f["interior_count"], f["arm"], f["apical"], f["arms"],
                                   f["stem_len"], f["ugu"], f["mfe"], f["pair_state"], f["percent"], f["bindings"]]
    return pruned, feat, f


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    tmp, rp, sc = load_reference(sys.argv[1])
    shared = ("main", "mapped", "hand_empty")   # (their texts are predict_precursors.json's)
    worlds = [(w["name"], w["features"], w["precursors"]) for w in json.load(open(PRECURSORS))["worlds"] if w["name"] in shared]
    worlds.append(("screen_hand",) + cases.hand_world())
    out, seen = [], set()
    try:
        for k, (name, features, fasta) in enumerate(worlds):
            d = os.path.join(tmp, "w%d" % k)
            os.mkdir(d)
            path = os.path.join(d, TABLE)
            with open(path, "w") as fh:
                fh.write(features)
            str_text = renamed(fasta, fold_texts(fasta))
            with open(path[:-4] + "_precusor.str", "w") as fh:
                fh.write(str_text)
            sc.screen_precusor_candidates(path, path[:-4] + "_precusor.str", 15, STANDIN)
            table = open(path[:-4] + model.UPDATED_SUFFIX).read()
            assert model.screen(features, str_text, fold_many) == table, "%s: the model's table and the reference's disagree" % name
            got = properties(features, str_text)
            if name == "screen_hand":
                seen = got
            lines = features.splitlines(True)
            tails = [row[len(line.strip()) + 1:] for line, row in zip(lines[1:], table.splitlines()[1:])]
            assert table == "".join([lines[0].strip() + "\t" + model.HEADER_TAIL] + [ln.strip() + "\t" + t + "\n" for ln, t in zip(lines[1:], tails)])
            folds = str_text.splitlines()[2::3]
            assert cases.str_of(fasta, folds) == str_text
            out.append(dict(name=name, sha256=cases.text_digest(features + fasta), folds=folds, tails=tails, holds=sorted(got)))
            print("%-12s %3d lines: %s" % (name, features.count("\n") - 1, " ".join(sorted(got))))
        for case in sorted(WANTED):
            assert case in seen, "the hand world does not hold: %s" % case
        rows, covered = [], set()
        inputs = cases.case_inputs()
        for seq, structure, mirnas in inputs:
            pruned, feat = run_case(rp, tmp, seq, structure, mirnas)
            m_pruned, m_feat, f = model_case(seq, structure, mirnas)
            if isinstance(feat, dict) or isinstance(pruned, dict):   # (the generator makes no call the reference dies of)
                raise AssertionError("the reference raised %r %r on %r" % (pruned, feat, (seq, structure, mirnas)))
            assert m_pruned == pruned and m_feat == feat, "the model disagrees on %r: %r %r, reference %r %r" % (
                (seq, structure, mirnas), m_pruned, m_feat, pruned, feat)
            covered |= case_properties(seq, structure, mirnas, pruned, f)
            rows.append(cases.pack_case(seq, mirnas, pruned, feat))
            assert cases.unpack_case(seq, mirnas, rows[-1]) == (pruned, feat), "the short form loses something of %r" % ((pruned, feat),)
        for case in sorted(CASE_WANTED):
            assert case in covered, "no case covers: %s" % case
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    with open(OUT, "w") as fh:
        json.dump(dict(source="reference utils/screen_precusor_candidates.py, classes/readPrecusor.py and forgi under lib2to3 "
                              "(Python 3: dictionaries keep insertion order); Bio.Seq stood in for; folds by tests/fold_standin.py",
                       inputs_sha256=cases.inputs_digest(inputs), worlds=out, cases=rows), fh, separators=(",", ":"))
    print("wrote %s: %d worlds, %d cases, %d bytes" % (OUT, len(out), len(rows), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
