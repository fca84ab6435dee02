#!/usr/bin/env python3
"""Capture tests/golden/predict_report.json from the REFERENCE's own utils/write_novel_report.py.

    python tests/golden/make_predict_report_golden.py <reference src/mirge directory>

Run only in the build container: the module is copied to a scratch directory outside the repository, converted with lib2to3
and imported from there next to stand-ins this script provides for `reportlab` and `Bio` (`Seq(...).transcribe()` = T to U).
The fold command handed in does nothing, and `creatPDF` is swapped for a recorder that keeps its arguments: nothing is drawn.
Only data is written into the repository, per world of tests/predict_report_cases.WORLDS:

  inputs     the three input texts (the small worlds) or their SHA-256 (the rest; the tests rebuild them from the generator)
  corrected  the reference's `_corrected.tsv`, as text or SHA-256
  report     the reference's `_novel_miRNAs_report.csv`, as text or SHA-256
  calls      the scalar arguments and the matureReadContentlist / passengerReadContentlist of every creatPDF call (the small
             worlds), and for every world the SHA-256 of their canonical form (tests/predict_report_cases.calls_form), which
             the tests read back from the report and the profile file
  holds      which of WANTED the world holds

main() asserts that tests/predict_report_model.py reproduces all of it, that the reference finished every world, and that
every case of WANTED is held by some world.
"""
import importlib
import json
import os
import shutil
import subprocess
import sys
import tempfile
import types

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import predict_report_cases as cases  # noqa: E402
from tests import predict_report_model as rule  # noqa: E402

OUT = os.path.join(HERE, "predict_report.json")
WANTED = {"offer_upstream", "offer_downstream", "both_offers_to_one_line", "first_line_offers_to_header", "retyped_to_loop", "already_loop",
          "cluster_seq_absent", "close_before_open_only", "group_of_1", "group_of_2", "group_of_3", "group_of_4", "group_of_5",
          "both_listed_first_larger", "both_listed_second_larger", "both_listed_tie", "only_first_listed", "only_second_listed",
          "passenger_dropped_for_loop", "mature_loop_skipped", "strand_plus", "strand_minus", "negative_pad", "ragged_row",
          "repeated_name_in_list"}
CALL_KEYS = ("name", "probability", "chr", "start", "end", "strand", "arm", "mature_reads", "total_reads", "precursor", "structure", "mature",
             "passenger", "mature_rows", "passenger_rows")


def load_reference(src):
    tmp = tempfile.mkdtemp(prefix="predict_report_golden_")
    root = os.path.join(tmp, "mirge_ref")
    os.makedirs(os.path.join(root, "utils"))
    for d in (root, os.path.join(root, "utils")):
        open(os.path.join(d, "__init__.py"), "w").close()
    with open(os.path.join(src, "utils", "write_novel_report.py"), "rb") as fh:
        data = fh.read().replace(b"\r\n", b"\n")
    with open(os.path.join(root, "utils", "write_novel_report.py"), "wb") as fh:
        fh.write(data)
    subprocess.run([sys.executable, "-m", "lib2to3", "-w", "-n", root], capture_output=True, check=True)
    for name in ("reportlab", "reportlab.lib", "reportlab.lib.colors", "reportlab.pdfgen", "reportlab.pdfgen.canvas", "reportlab.lib.pagesizes",
                 "Bio", "Bio.Seq", "Bio.Alphabet"):
        sys.modules[name] = types.ModuleType(name)
    sys.modules["reportlab.lib"].colors = sys.modules["reportlab.lib.colors"]
    sys.modules["reportlab.pdfgen"].canvas = sys.modules["reportlab.pdfgen.canvas"]
    sys.modules["reportlab.lib.pagesizes"].A4 = (595.27, 841.89)

    class Seq(object):
        def __init__(self, text, alphabet=None):
            self.text = text

        def transcribe(self):
            return self.text.replace("T", "U")

        def __str__(self):
            return self.text
    Seq.transcribe = lambda self: Seq(self.text.replace("T", "U"))
    sys.modules["Bio.Seq"].Seq = Seq
    sys.modules["Bio.Alphabet"].generic_dna = None
    sys.path.insert(0, tmp)
    return tmp, importlib.import_module("mirge_ref.utils.write_novel_report")


def run_reference(mod, tmp, k, texts):
    d = os.path.join(tmp, "w%d" % k)
    os.mkdir(d)
    paths = [os.path.join(d, nm) for nm in (cases.NOVEL, cases.TABLE, cases.CLUSTER)]
    for p, text in zip(paths, texts):
        with open(p, "w") as fh:
            fh.write(text)
    calls = []

    def recorder(sampleName, name, probability, chr, startPos, endPos, strand, armType, matureReads, totalReads, precursor, structure, mature,
                 passenger, psFile, outFile, matureRows, passengerRows):
        rows = lambda r: r if r == "None" else [[t, int(c)] for t, c in r]
        calls.append(dict(name=name, probability=probability, chr=chr, start=startPos, end=endPos, strand=strand, arm=armType,
                          mature_reads=matureReads, total_reads=totalReads, precursor=precursor, structure=structure, mature=mature,
                          passenger=passenger, mature_rows=rows(matureRows), passenger_rows=rows(passengerRows)))
    mod.creatPDF = recorder
    mod.write_novel_report(paths[0], paths[1], paths[2], "true")
    out = rule.output_paths(*paths)
    with open(out["corrected"]) as fh:
        corrected = fh.read()
    with open(out["report"]) as fh:
        report = fh.read()
    return corrected, report, calls


def holds(texts, res):
    """Which of WANTED a world holds, from the model's results over it."""
    names, prob = rule.parse_novel(texts[0])
    t = rule.Table(texts[1], names)
    n = t.n
    got = set()
    listed = [t.col(j, "clusterName") in prob for j in range(n)]
    quals = [listed[j] and t.col(j, "pair_state") == "Yes" and t.up[j] != rule.NONE for j in range(n)]
    up_offer = [quals[j] and t.up[j] <= 44 for j in range(n)]
    down_offer = [quals[j] and t.up[j] > 44 and t.down[j] <= 44 for j in range(n)]
    src = res["src"].tolist()
    if any(src[j] == j + 1 for j in range(n)):
        got.add("offer_upstream")
    if any(src[j] == j - 1 for j in range(n)):
        got.add("offer_downstream")
    if any(0 < j < n - 1 and down_offer[j - 1] and up_offer[j + 1] and src[j] == j + 1 for j in range(n)):
        got.add("both_offers_to_one_line")
    if n and up_offer[0]:
        got.add("first_line_offers_to_header")
    state = res["state"].tolist()
    if any(s & 2 for s in state):
        got.add("retyped_to_loop")
    for j in range(n):
        seq, structure = t.col(src[j], "pruned_precusor_seq"), t.col(src[j], "pruned_precusor_str")
        rna = t.col(j, "clusterSeq").replace("T", "U")
        at = seq.find(rna)
        stretch = structure[at:at + len(rna)]
        if t.col(j, "armType") == "loop" and rule.retype(seq, structure, t.col(j, "clusterSeq")):
            got.add("already_loop")
        if at < 0 and seq != "None":
            got.add("cluster_seq_absent")
        if ")" in stretch and "(" in stretch and stretch.rindex(")") < stretch.index("("):
            got.add("close_before_open_only")
    sizes = {}
    for j in range(n):
        if not state[j] & 8:
            key = (t.col(src[j], "pruned_precusor_seq"), t.chr[j], t.strand[j])
            sizes.setdefault(key, []).append(j)
    visited = set()
    for m, p in res["chunks"]:
        key = (t.col(src[m], "pruned_precusor_seq"), t.chr[m], t.strand[m])
        visited.add(key)
    for key in visited:
        if 1 <= len(sizes[key]) <= 5:
            got.add("group_of_%d" % len(sizes[key]))
        members = sizes[key]
        for k in range(0, len(members) - 1, 2):
            a, b = members[k], members[k + 1]
            if listed[a] and listed[b]:
                got.add("both_listed_tie" if t.reads[a] == t.reads[b] else "both_listed_first_larger" if t.reads[a] > t.reads[b] else "both_listed_second_larger")
            elif listed[a]:
                got.add("only_first_listed")
            elif listed[b]:
                got.add("only_second_listed")
    arm = lambda j: "loop" if state[j] & 2 else t.col(j, "armType")
    for m, p in res["chunks"]:
        key = (t.col(src[m], "pruned_precusor_seq"), t.chr[m], t.strand[m])
        members = sizes[key]
        at = members.index(m) // 2 * 2
        if p is None and len(members[at:at + 2]) == 2:
            got.add("passenger_dropped_for_loop")
        if arm(m) == "loop":
            got.add("mature_loop_skipped")
    for c in res["calls"]:
        got.add("strand_plus" if c["strand"] == "+" else "strand_minus")
    if res["flag"].size and (res["flag"] & 1).any():
        got.add("ragged_row")
    # a negative pad: a row shorter than its two pads and its bases would make it without the clamp
    for e, c in enumerate(res["calls"]):
        m, p = int(res["ent_m"][e]), int(res["ent_p"][e])
        L = len(c["precursor"])
        rows = c["mature_rows"] + ([] if c["passenger_rows"] == "None" else c["passenger_rows"])
        if any(len(r[0]) > L and (r[0][0] != "-" or r[0][-1] != "-") for r in rows):
            got.add("negative_pad")
    if len(rule.lines_of(texts[0])) - 1 > len(names):
        got.add("repeated_name_in_list")
    return got


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    tmp, mod = load_reference(sys.argv[1])
    worlds, seen = [], set()
    try:
        for k, name in enumerate(cases.WORLDS):
            texts = cases.world(name)
            corrected, report, calls = run_reference(mod, tmp, k, texts)   # (the reference finished: it did not raise)
            mine = rule.run(*texts)
            assert mine["corrected"] == corrected, "%s: the reference's corrected table and the model's disagree" % name
            assert mine["report"] == report, "%s: the reference's report and the model's disagree" % name
            assert len(mine["calls"]) == len(calls) == report.count("\n") - 1, name
            for a, b in zip(mine["calls"], calls):
                for key in CALL_KEYS:
                    assert str(a[key]) == str(b[key]) if key in ("start", "end", "mature_reads", "total_reads") else a[key] == b[key], (name, key, a[key], b[key])
            got = holds(texts, mine)
            seen |= got
            as_text = name in cases.TEXT_WORLDS
            keep = (lambda s: s) if as_text else cases.digest
            form = cases.calls_form(calls)
            assert form == cases.calls_form_from_files(mine["report"], mine["profiles"]), "%s: the files do not give the recorded calls back" % name
            worlds.append(dict(name=name, as_text=as_text, inputs=[keep(s) for s in texts], corrected=keep(corrected), report=keep(report),
                               calls=[{key: c[key] for key in CALL_KEYS} for c in calls] if as_text else None, n_calls=len(calls),
                               calls_sha256=cases.calls_digest(form), holds=sorted(got)))
            print("%-16s %4d lines, %3d entries: %s" % (name, len(rule.lines_of(texts[1])) - 1, len(calls), " ".join(sorted(got))))
        for case in sorted(WANTED):
            assert case in seen, "no world holds: %s" % case
        for name, texts in cases.raising_cases().items():   # the reference raises on each of the hand-made inputs, and so does the model
            try:
                run_reference(mod, tmp, 100 + len(name), texts)
            except Exception as e:
                print("%-40s the reference raises %s" % (name, type(e).__name__))
            else:
                raise AssertionError("%s: the reference does not raise" % name)
            try:
                rule.run(*texts)
            except ValueError:
                pass
            else:
                raise AssertionError("%s: the model does not raise" % name)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    with open(OUT, "w") as fh:
        json.dump(dict(source="reference utils/write_novel_report.py under lib2to3, creatPDF recorded, nothing drawn", worlds=worlds), fh,
                  separators=(",", ":"))
    print("wrote %s: %d worlds, %d bytes" % (OUT, len(worlds), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
