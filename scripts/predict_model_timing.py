#!/usr/bin/env python3
"""Timing of predict mode's classification (miRge2.0.py:647-648) on a screened table of about --rows retained rows that
tests/predict_model_cases.timing_text builds around the support vectors of the human model (the fixture's arrays).  Both
laps start with `*_features_updated_stableClusterSeq_15.tsv` on disk and end with the five files closed:

  (a) the rule in Python over the same text (tests/predict_model_model.run: the filters on text, numpy float64 with the
      sequential sum, the coupling loop per row) and a plain writer; where sklearn imports on this machine, its
      decision_function and predict_proba over the same rows are timed too (the model filled as the fixture's maker does);
  (b) predict.classify_candidates: the native reader and its three filter files, Engine.predict_svm (upload, one launch,
      download) and the native writer, each timed; the launch alone between device events.

Each route runs once as a warm-up and then --runs times in this one process.  The filter files of the two routes must be
equal and the numbers agree within the tests' tolerance.  No ratio is fixed in advance.  Writes one JSON object to --json,
default profiles/predict_model_timing.json, and prints it."""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def spread(xs):
    return dict(min=round(min(xs), 6), max=round(max(xs), 6))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "predict_model_timing.json"))
    args = ap.parse_args()
    import torch
    from mirge_amd import predict
    from mirge_amd.engine import Engine
    from tests import predict_model_cases as cases
    from tests import predict_model_model as rule
    model = cases.fixture_model()
    namelist = cases.golden()["namelist"]
    text = cases.timing_text(model, args.rows)
    res = dict(what="predict mode: the SVM over the screened table", rows=args.rows, runs=args.runs, model="human: %d support vectors, %d features" % model.sv.shape,
               table_bytes=len(text))
    eng = Engine(0)
    try:
        with tempfile.TemporaryDirectory() as d:
            path = os.path.join(d, cases.TABLE)
            with open(path, "w") as fh:
                fh.write(text)
            paths = predict.classified_paths(path)
            # (a) the rule
            laps_a, want = [], None
            for k in range(args.runs + 1):
                t0 = time.perf_counter()
                want = rule.run(text, namelist, model)
                for key in paths:
                    with open(paths[key] + ".rule", "w") as fh:
                        fh.write(want[key])
                if k:
                    laps_a.append(time.perf_counter() - t0)
            res["a_rule_s"] = spread(laps_a)
            res["retained_rows"] = int(len(want["x"]))
            res["predicted_1"], res["kept"] = int((want["pred"] == 1).sum()), want["novel"].count("\n") - 1
            # (b) the array route
            laps_b, parts = [], []
            for k in range(args.runs + 1):
                timings = {}
                t0 = time.perf_counter()
                got = predict.classify_candidates(eng, path, None, None, classifier=(model, namelist), timings=timings)
                if k:
                    laps_b.append(time.perf_counter() - t0)
                    parts.append(timings)
            res["b_array_route_s"] = spread(laps_b)
            res["b_split_s"] = {key: spread([p[key] for p in parts]) for key in ("read_s", "device_s", "write_s")}
            for key in ("dataset", "refined_tmp", "refined"):
                with open(paths[key]) as fh:
                    assert fh.read() == want[key], key
            t = rule.tolerance(model)
            res["max_decision_difference"] = float(np.abs(got["dec"] - want["dec"]).max())
            res["max_probability_difference"] = float(np.abs(got["prob"] - want["prob"]).max())
            res["tolerance"] = t
            assert res["max_decision_difference"] <= t
            res["files_equal"] = True
            # the launch alone
            dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64).reshape(-1)).to(eng.device)
            x, mean, scale, sv, coef = dev(want["x"]), dev(model.mean), dev(model.scale), dev(model.sv), dev(model.coef)
            n = len(want["x"])
            pred = torch.empty(n, dtype=torch.int8, device=eng.device)
            dec, prob = torch.empty(n, dtype=torch.float64, device=eng.device), torch.empty(2 * n, dtype=torch.float64, device=eng.device)
            ms = []
            for k in range(args.runs + 1):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                rc = eng._lib.mrg_predict_svm(eng._h, n, x.data_ptr(), model.sv.shape[1], mean.data_ptr(), scale.data_ptr(), sv.data_ptr(),
                                              coef.data_ptr(), model.sv.shape[0], model.intercept, model.gamma, model.probA, model.probB,
                                              pred.data_ptr(), dec.data_ptr(), prob.data_ptr(), eng._stream_ptr())
                e1.record()
                e1.synchronize()
                assert rc == 0
                if k:
                    ms.append(e0.elapsed_time(e1))
            res["b_launch_ms"] = spread(ms)
            # sklearn, where it imports
            try:
                sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
                from make_predict_model_golden import sklearn_objects
                sc, pipe, _ = sklearn_objects(model)
                laps = []
                for k in range(args.runs + 1):
                    t0 = time.perf_counter()
                    z = sc.transform(want["x"])
                    pipe.predict(z)
                    pipe.predict_proba(z)
                    if k:
                        laps.append(time.perf_counter() - t0)
                res["sklearn_predict_and_proba_s"] = spread(laps)
            except ImportError:
                res["sklearn_predict_and_proba_s"] = None
    finally:
        eng.close()
    res["ratio_b_over_a"] = round(res["b_array_route_s"]["min"] / res["a_rule_s"]["min"], 5)
    res["command"] = "python scripts/predict_model_timing.py --rows %d --runs %d" % (args.rows, args.runs)
    os.makedirs(os.path.dirname(args.json), exist_ok=True)
    with open(args.json, "w") as fh:
        json.dump(res, fh)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
