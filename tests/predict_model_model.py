"""The rule of predict mode's classification (reference utils/preprocess_featureFiles.py and utils/model_predict.py with
libsvm's svm_predict_probability behind them), restated: the three filters as plain Python on text, the feature matrix
pandas' read_csv / get_dummies lead to, and the SVM in numpy float64 with the sum over the support vectors in their stored
order and libsvm's coupling iteration per row.  tests/golden/make_predict_model_golden.py holds this module against the
reference's two modules run over sklearn; the tests hold the engine against it.
"""
import math
import os

import numpy as np

READ_COUNT_LIMIT, SEQ_COUNT_LIMIT, CUTOFF = 10, 3, 0.8
MIN_PROB = 1e-7
COUPLING_EPS, COUPLING_MAX_ITER = 0.005 / 2, 100


# ------------------------------------------------------------------------------------------------ names
def tmp_name(table_path):
    base = os.path.basename(table_path)
    return "_".join(base.split("_")[:-9]) + "_dataset_" + base.split("_")[-1].split(".")[0]


def sample_name(table_path):
    return "_".join((tmp_name(table_path) + "_refined_features.csv").split("_")[2:-5])


def output_paths(table_path):
    """The five files, in the order they are written."""
    d, tmp = os.path.dirname(table_path), tmp_name(table_path)
    s = sample_name(table_path)
    return dict(dataset=os.path.join(d, tmp + ".csv"), refined_tmp=os.path.join(d, tmp + "_refined_tmp.csv"),
                refined=os.path.join(d, tmp + "_refined_features.csv"), detailed=os.path.join(d, "predicted_" + s + "_detailed.csv"),
                novel=os.path.join(d, s + "_novel_miRNAs_miRge2.0.csv"))


# ------------------------------------------------------------------------------------------------ the filters
def filter_texts(table, namelist):
    """(dataset text, refined_tmp text, refined_features text) of a screened table's text."""
    lines = table.splitlines(True)
    if not lines:
        raise ValueError("no header line")
    head = lines[0].strip().split("\t")
    keep = [i for i in range(len(head)) if i in (0, 1, 5) or i >= 10]
    i_reads, i_seqs = head.index("readCountSum"), head.index("seqCount")
    first = [",".join(head[i] for i in keep) + "\n"]
    for line in lines[1:]:
        c = line.strip().split("\t")
        if int(c[i_reads]) >= READ_COUNT_LIMIT and int(c[i_seqs]) >= SEQ_COUNT_LIMIT and "N" not in c[i_seqs:]:
            first.append(",".join(c[i] for i in keep if i < len(c)) + "\n")
    h1 = first[0].strip().split(",")
    i_str = h1.index("pruned_precusor_str")
    second = [first[0]] + [ln for ln in first[1:] if ln.strip().split(",")[i_str] != "None"]
    names = []
    for n in namelist:
        if n.strip() not in names:
            names.append(n.strip())
    cols = [i for i, n in enumerate(h1) if n in names]
    third = [",".join(h1[i] for i in cols) + "\n"]
    for ln in second[1:]:
        c = ln.strip().split(",")
        third.append(",".join(c[i] for i in cols if i < len(c)) + "\n")
    return "".join(first), "".join(second), "".join(third)


# ------------------------------------------------------------------------------------------------ the feature matrix
def _number(cell):
    """A cell of a column of numbers: digits, signs, a point and an exponent that float() reads; None for anything else (an
    empty cell, a word, `nan`, `inf`)."""
    t = cell.strip()
    if not t or any(ch not in "0123456789+-.eE" for ch in t):
        return None
    try:
        return float(t)
    except ValueError:
        return None


def feature_matrix(refined, feature_names):
    """(names [n][3] as text, X [n][nf] float64, the selected names whose column holds a non-numeric cell) of the refined
    features text.  A selected name is, in this order: a column of numbers; `<column>_<value>` of a column that is not one
    (1.0 where the cell equals the value); absent, a column of 0."""
    lines = refined.splitlines()
    head = lines[0].split(",") if lines else []
    rows = [ln.strip().split(",") for ln in lines[1:]]
    for r in rows:
        if len(r) != len(head):
            raise ValueError("a line of %d cells under a header of %d" % (len(r), len(head)))
    names = [r[:3] for r in rows]
    numeric = {}
    for ci in range(3, len(head)):
        vals = [_number(r[ci]) for r in rows]
        numeric[ci] = None if any(v is None for v in vals) else vals
    x = np.zeros((len(rows), len(feature_names)), np.float64)
    stray = []
    for fi, f in enumerate(feature_names):
        hit = [ci for ci in range(3, len(head)) if head[ci] == f]
        if hit and numeric[hit[0]] is not None:
            x[:, fi] = numeric[hit[0]]
            continue
        if hit and rows:
            stray.append(f)
        for ci in range(3, len(head)):
            if numeric[ci] is None and f.startswith(head[ci] + "_") and any(r[ci] == f[len(head[ci]) + 1:] for r in rows):
                x[:, fi] = [1.0 if r[ci] == f[len(head[ci]) + 1:] else 0.0 for r in rows]
                break
    return names, x, stray


# ------------------------------------------------------------------------------------------------ the SVM
def tolerance(model):
    """T of the issue: the worst case of adding the terms of the decision sum in another order."""
    return 4.0 * 2.0 ** -53 * len(model.coef) * float(np.abs(model.coef).sum())


def standardise(model, x):
    return (np.asarray(x, np.float64) - model.mean) / model.scale


def decision(model, x):
    """The decision values of raw rows x [n][nf]: for every row the terms coef_i exp(-gamma |z - sv_i|^2) added one support
    vector after the other in their stored order, the intercept last."""
    z = standardise(model, x)
    total = np.zeros(len(z), np.float64)
    for i in range(len(model.coef)):
        d = z - model.sv[i]
        dist = np.zeros(len(z), np.float64)
        for j in range(d.shape[1]):
            dist = dist + d[:, j] * d[:, j]
        total = total + model.coef[i] * np.exp(-model.gamma * dist)
    return total + model.intercept


def sigmoid(f, a, b):
    """libsvm's sigmoid_predict."""
    v = f * a + b
    if v >= 0:
        e = math.exp(-v)
        return e / (1.0 + e)
    return 1.0 / (1.0 + math.exp(v))


def couple(r01):
    """libsvm's multiclass_probability for two classes from the pairwise probability r01 of the first.  Returns
    (p0, p1, rounds, the stopping quantity of every round that was tested)."""
    r10 = 1.0 - r01
    q00, q11 = r10 * r10, r01 * r01
    q01 = -r10 * r01
    q = ((q00, q01), (q01, q11))
    p = [0.5, 0.5]
    errors = []
    rounds = 0
    for rounds in range(COUPLING_MAX_ITER):
        qp = [q[0][0] * p[0] + q[0][1] * p[1], q[1][0] * p[0] + q[1][1] * p[1]]
        pqp = p[0] * qp[0] + p[1] * qp[1]
        err = max(abs(qp[0] - pqp), abs(qp[1] - pqp))
        errors.append(err)
        if err < COUPLING_EPS:
            break
        for t in range(2):
            diff = (-qp[t] + pqp) / q[t][t]
            p[t] += diff
            pqp = (pqp + diff * (diff * q[t][t] + 2 * qp[t])) / (1 + diff) / (1 + diff)
            for j in range(2):
                qp[j] = (qp[j] + diff * q[t][j]) / (1 + diff)
                p[j] /= (1 + diff)
    else:
        rounds = COUPLING_MAX_ITER
    return p[0], p[1], rounds, errors


def classify(model, x):
    """dict of arrays over the rows: dec, pred (int8, 1 or -1), prob [n][2] (class -1, class 1), rounds, clipped, errors."""
    dec = decision(model, x)
    n = len(dec)
    pred = np.where(dec < 0, -1, 1).astype(np.int8)
    prob = np.zeros((n, 2), np.float64)
    rounds = np.zeros(n, np.int32)
    clipped = np.zeros(n, bool)
    errors = []
    for k in range(n):
        # libsvm's own decision value is sklearn's negated; its first class is -1
        s = sigmoid(-float(dec[k]), model.probA, model.probB)
        r = min(max(s, MIN_PROB), 1.0 - MIN_PROB)
        clipped[k] = r != s
        p0, p1, rounds[k], err = couple(r)
        prob[k] = (p0, p1)
        errors.append(err)
    return dict(dec=dec, pred=pred, prob=prob, rounds=rounds, clipped=clipped, errors=errors)


# ------------------------------------------------------------------------------------------------ the two result files
def result_texts(header3, names, pred, prob):
    """(detailed text, novel text): pred [n], prob [n][2]; the probability printed is the larger of a row's two."""
    head = "predictedValue,probability," + ",".join(header3) + "\n"
    lines = ["%d,%r,%s\n" % (int(pred[k]), float(max(prob[k])), ",".join(names[k])) for k in range(len(names))]
    kept = []
    for ln in lines:
        c = ln.strip().split(",")
        if c[0] == "1" and float(c[1]) >= CUTOFF:
            kept.append([float(c[1]), ln])
    kept.sort(reverse=True)
    return head + "".join(lines), head + "".join(ln for _, ln in kept)


def run(table, namelist, model):
    """Everything from a screened table's text: dict of the five texts (output_paths' keys), the feature rows x, the selected
    names with a stray cell, the rows' three leading cells (names_of_rows) and classify's arrays."""
    dataset, refined_tmp, refined = filter_texts(table, namelist)
    names, x, stray = feature_matrix(refined, model.feature_names)
    res = classify(model, x)
    header3 = refined.splitlines()[0].split(",")[:3]
    detailed, novel = result_texts(header3, names, res["pred"], res["prob"])
    return dict(dataset=dataset, refined_tmp=refined_tmp, refined=refined, detailed=detailed, novel=novel, x=x, stray=stray,
                names_of_rows=names, **res)
