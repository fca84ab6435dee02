#!/usr/bin/env python3
"""Capture tests/golden/predict_model.json from the REFERENCE's own utils/preprocess_featureFiles.py and
utils/model_predict.py, run over this machine's pandas and sklearn.

    python tests/golden/make_predict_model_golden.py <reference src/mirge directory>

Run only in the build container: the two modules are copied to a scratch directory outside the repository, converted with
lib2to3 and imported from there next to stand-ins this script provides: matplotlib where it is absent, and
`sklearn.externals.joblib`, whose `load` fills this machine's StandardScaler and SVC from the arrays mirge_amd.svm_model
reads out of the model file (the file was written by sklearn 0.18.1 and no longer unpickles).  Only data is written into the
repository:

  model     the human model's arrays (float64, deflated, base64) and its selected names: what the tests classify with
  files     the SHA-256 of the three model files and of the arrays our reader returns from each
  namelist  the lines of total_features_namelist.txt
  worlds    per world of tests/predict_model_cases.WORLDS: the rows left out as open (closer than a margin to a threshold:
            cases.open_rows; at most 1 % may be), the SHA-256 of the table text and of the reference's five files, the
            `predictedValue,probability` fields of every line of its detailed file, the lines of its novel list as indices
            into the detailed file, and what the world holds.  WANTED names what the worlds must hold; main() asserts it.

main() also asserts that tests/predict_model_model.py agrees with the reference: the three filter files byte for byte, the
labels exactly, decision values against sklearn's decision_function within T = cases' tolerance and probabilities within
T max(1, |A| / 4), the novel list's rows and order.

One thing no row of a world can hold with this model, so the hand-made models of tests/test_gpu_predict_model.py and the
writer's tests cover it: a KEPT row whose larger probability is class -1's.  A row predicted 1 has a decision value of 0 or
more, where class -1's probability is at most 1 / (1 + exp(B)) = 0.559 with this model's B = -0.236; the worlds hold such
rows, but none of them can reach 0.8.

main() also runs a plain table near the support vectors of the mouse and the others model through the reference with the
stand-in loader and asserts the same agreement, so a transposed or mis-ordered read of either file would show; `files` keeps
the counts.
"""
import hashlib
import importlib
import json
import os
import shutil
import subprocess
import sys
import tempfile
import types
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from mirge_amd import svm_model  # noqa: E402
from tests import predict_model_cases as cases  # noqa: E402
from tests import predict_model_model as rule  # noqa: E402

OUT = os.path.join(HERE, "predict_model.json")
WANTED = {"clip", "clip_high", "clip_low", "kept", "predicted_1_below_cutoff", "predicted_1_with_larger_probability_of_minus_1", "rounds_0", "rounds_1", "rounds_2",
          "count_below_10", "fewer_than_3_sequences", "cell_equal_N", "cell_containing_N", "none_structure", "counts_at_the_limits",
          "N_before_seqCount", "selected_name_absent", "stray_string"}
_LOADED = {}


def sklearn_objects(m):
    """[StandardScaler, Pipeline([('clf', SVC)]), selected] of this machine's sklearn, filled from a SvmModel."""
    from sklearn.pipeline import Pipeline
    from sklearn.preprocessing import StandardScaler
    from sklearn.svm import SVC
    n, nf = m.sv.shape
    sc = StandardScaler()
    sc.mean_, sc.scale_, sc.var_, sc.n_features_in_, sc.n_samples_seen_ = m.mean, m.scale, m.scale ** 2, nf, 1
    svc = SVC(kernel="rbf", gamma=m.gamma, probability=True)
    n_pos = int((m.coef > 0).sum())
    svc.support_vectors_, svc.support_ = m.sv, np.arange(n, dtype=np.int32)
    svc._n_support = np.array([n - n_pos, n_pos], dtype=np.int32)
    svc.dual_coef_ = m.coef[None, :].copy()
    svc._dual_coef_ = -svc.dual_coef_
    svc.intercept_ = np.array([m.intercept])
    svc._intercept_ = -svc.intercept_
    svc._probA, svc._probB, svc._gamma, svc._sparse = np.array([m.probA]), np.array([m.probB]), m.gamma, False
    svc.shape_fit_, svc.class_weight_, svc.classes_, svc.n_features_in_, svc.fit_status_ = (n, nf), np.ones(2), np.array([-1, 1]), nf, 0
    return [sc, Pipeline([("clf", svc)]), [(0.0, j, f) for j, f in enumerate(m.feature_names)]]


def load_reference(src):
    tmp = tempfile.mkdtemp(prefix="predict_model_golden_")
    root = os.path.join(tmp, "mirge_ref")
    os.makedirs(os.path.join(root, "utils"))
    for d in (root, os.path.join(root, "utils")):
        open(os.path.join(d, "__init__.py"), "w").close()
    for name in ("preprocess_featureFiles.py", "model_predict.py"):
        with open(os.path.join(src, "utils", name), "rb") as fh:
            data = fh.read().replace(b"\r\n", b"\n")
        with open(os.path.join(root, "utils", name), "wb") as fh:
            fh.write(data)
    subprocess.run([sys.executable, "-m", "lib2to3", "-w", "-n", root], capture_output=True, check=True)
    try:
        importlib.import_module("matplotlib")
    except ImportError:
        for name in ("matplotlib", "matplotlib.pyplot", "matplotlib.backends", "matplotlib.backends.backend_pdf"):
            sys.modules[name] = types.ModuleType(name)
        sys.modules["matplotlib"].use = lambda *a, **k: None
        sys.modules["matplotlib"].pyplot = sys.modules["matplotlib.pyplot"]
        sys.modules["matplotlib.backends.backend_pdf"].PdfPages = object
    joblib = types.ModuleType("sklearn.externals.joblib")
    joblib.load = lambda path: sklearn_objects(_LOADED[path])
    import sklearn.externals
    sys.modules["sklearn.externals.joblib"] = joblib
    sklearn.externals.joblib = joblib
    sys.path.insert(0, tmp)
    return tmp, importlib.import_module("mirge_ref.utils.preprocess_featureFiles"), importlib.import_module("mirge_ref.utils.model_predict")


def file_digest(path):
    with open(path, "rb") as fh:
        return hashlib.sha256(fh.read()).hexdigest()


def arrays_digest(m):
    h = hashlib.sha256()
    for a in (m.mean, m.scale, m.sv, m.coef, np.array([m.intercept, m.gamma, m.probA, m.probB])):
        h.update(np.ascontiguousarray(a, dtype="<f8").tobytes())
    h.update("\n".join(m.feature_names).encode())
    return h.hexdigest()


def run_reference(pre, mp, tmp, k, text, namelist_path, model_path):
    d = os.path.join(tmp, "w%d" % k)
    os.mkdir(d)
    path = os.path.join(d, cases.TABLE)
    with open(path, "w") as fh:
        fh.write(text)
    pre.preprocess_featureFiles(path, namelist_path)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        mp.model_predict(path, model_path)
    out = {}
    for key, p in rule.output_paths(path).items():
        with open(p) as fh:
            out[key] = fh.read()
    return out


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    src = sys.argv[1]
    models_dir = os.path.join(src, "models")
    files = {}
    for species in ("human", "mouse", "others"):
        path = svm_model.model_path(models_dir, species)
        _LOADED[path] = svm_model.load_model(models_dir, species)
        files[species] = dict(sha256=file_digest(path), arrays_sha256=arrays_digest(_LOADED[path]))
    human_path = svm_model.model_path(models_dir, "human")
    m = _LOADED[human_path]
    assert arrays_digest(cases.model_from_json(cases.model_to_json(m))) == arrays_digest(m), "the fixture's form loses something of the model"
    namelist = svm_model.read_namelist(models_dir)
    with open(os.path.join(models_dir, svm_model.NAMELIST)) as fh:
        namelist_lines = fh.read().splitlines()
    t = rule.tolerance(m)
    tp = cases.prob_margin(m, t)
    sc, pipe, _ = sklearn_objects(m)
    tmp, pre, mp = load_reference(src)
    worlds, seen = [], set()
    try:
        for n_check, species in enumerate(("mouse", "others")):   # the reader per model file, against sklearn over the reference
            path = svm_model.model_path(models_dir, species)
            mm = _LOADED[path]
            text = cases.species_text(mm)
            mine = rule.run(text, namelist, mm)
            ts = rule.tolerance(mm)
            assert not cases.open_rows(mm, mine, ts), "%s: open rows in the check table" % species
            ref = run_reference(pre, mp, tmp, 100 + n_check, text, os.path.join(models_dir, svm_model.NAMELIST), path)
            assert all(ref[key] == mine[key] for key in ("dataset", "refined_tmp", "refined")), species
            ref_lines, my_lines = ref["detailed"].splitlines(), mine["detailed"].splitlines()
            assert len(ref_lines) == len(my_lines) > 60
            for a, b in zip(ref_lines[1:], my_lines[1:]):
                ca, cb = a.split(","), b.split(",")
                assert ca[0] == cb[0] and ca[2:] == cb[2:] and abs(float(ca[1]) - float(cb[1])) <= cases.prob_margin(mm, ts), (species, a, b)
            assert [ln.split(",", 2)[2] for ln in ref["novel"].splitlines()] == [ln.split(",", 2)[2] for ln in mine["novel"].splitlines()]
            assert len(set(ln.split(",")[1] for ln in ref_lines[1:])) > 40, "%s: the check table's rows are all alike" % species
            files[species]["check"] = dict(rows=len(ref_lines) - 1, predicted_1=int((mine["pred"] == 1).sum()), kept=ref["novel"].count("\n") - 1)
            print("%-8s check: %s" % (species, files[species]["check"]))
        for k, (name, n, seed) in enumerate(cases.WORLDS):
            rows = cases.world_rows(m, name, n, seed)
            by_cluster = {r["clusterName"]: i for i, r in enumerate(rows)}
            assert len(by_cluster) == len(rows)
            first = rule.run(cases.table_text(rows), namelist, m)
            dropped = sorted(by_cluster[first["names_of_rows"][j][2]] for j in cases.open_rows(m, first, t))
            assert len(dropped) <= 0.01 * len(rows), "%s: %d of %d rows are open" % (name, len(dropped), len(rows))
            text = cases.table_text(rows, dropped)
            mine = rule.run(text, namelist, m)
            assert not cases.open_rows(m, mine, t), "%s: rows are open after the open rows were left out" % name
            ref = run_reference(pre, mp, tmp, k, text, os.path.join(models_dir, svm_model.NAMELIST), human_path)
            for key in ("dataset", "refined_tmp", "refined"):
                assert ref[key] == mine[key], "%s: the reference's %s file and the model's disagree" % (name, key)
            # the numbers: sklearn's against the restatement's
            dec = pipe.decision_function(sc.transform(mine["x"])) if len(mine["x"]) else np.zeros(0)
            assert np.abs(dec - mine["dec"]).max() <= t, "%s: decision values differ by %g, T = %g" % (name, np.abs(dec - mine["dec"]).max(), t)
            ref_lines, my_lines = ref["detailed"].splitlines(), mine["detailed"].splitlines()
            assert ref_lines[0] == my_lines[0] and len(ref_lines) == len(my_lines)
            fields = []
            for a, b in zip(ref_lines[1:], my_lines[1:]):
                ca, cb = a.split(","), b.split(",")
                assert ca[0] == cb[0] and ca[2:] == cb[2:], "%s: %r / %r" % (name, a, b)
                assert abs(float(ca[1]) - float(cb[1])) <= tp, "%s: probabilities %s / %s, margin %g" % (name, ca[1], cb[1], tp)
                assert repr(float(ca[1])) == ca[1]
                fields.append(ca[0] + "," + ca[1])
            ref_novel, my_novel = ref["novel"].splitlines(), mine["novel"].splitlines()
            assert ref_novel[0] == ref_lines[0]
            order = [ref_lines.index(ln) - 1 for ln in ref_novel[1:]]
            assert order == [my_lines.index(ln) - 1 for ln in my_novel[1:]], "%s: the novel lists differ in rows or order" % name
            # what the world holds
            got = set(r["_what"] for i, r in enumerate(rows) if i not in set(dropped)) - {"plain"}
            top = mine["prob"].max(axis=1)
            ones = mine["pred"] == 1
            if (ones & (top >= rule.CUTOFF)).any():
                got.add("kept")
            if (ones & (top < rule.CUTOFF)).any():
                got.add("predicted_1_below_cutoff")
            if (ones & (mine["prob"][:, 0] > mine["prob"][:, 1])).any():
                got.add("predicted_1_with_larger_probability_of_minus_1")
            got |= set("rounds_%d" % r for r in set(mine["rounds"].tolist()))
            if mine["clipped"].any():
                got.add("clip")
            head = mine["refined"].splitlines()[0].split(",")
            if name == "absent":
                assert not mine["x"][:, m.feature_names.index("armType_loop")].any() and not mine["x"][:, m.feature_names.index("pair_state_No")].any()
                got.add("selected_name_absent")
            if mine["stray"]:
                assert mine["stray"] == ["hairpin_count"] and "hairpin_count" in head and not mine["x"][:, m.feature_names.index("hairpin_count")].any()
            else:
                got.discard("stray_string")
            seen |= got
            worlds.append(dict(name=name, dropped=dropped, sha256=cases.text_digest(text), files={key: cases.text_digest(ref[key]) for key in ref},
                               rows=fields, novel=order, holds=sorted(got)))
            print("%-8s %4d rows, %d left out, %d retained, %d predicted 1, %d kept: %s" % (
                name, len(rows), len(dropped), len(fields), int(ones.sum()), len(order), " ".join(sorted(got))))
        for case in sorted(WANTED):
            assert case in seen, "no world holds: %s" % case
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    with open(OUT, "w") as fh:
        json.dump(dict(source="reference utils/preprocess_featureFiles.py and utils/model_predict.py under lib2to3, pandas %s, sklearn %s; "
                              "the model files read by mirge_amd.svm_model" % (importlib.import_module("pandas").__version__,
                                                                                 importlib.import_module("sklearn").__version__),
                       tolerance=repr(t), model=cases.model_to_json(m), files=files, namelist=namelist_lines, worlds=worlds), fh,
                  separators=(",", ":"))
    print("wrote %s: %d worlds, %d bytes" % (OUT, len(worlds), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
