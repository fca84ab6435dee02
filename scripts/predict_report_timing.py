#!/usr/bin/env python3
"""Timing of predict mode's report (miRge2.0.py:652 without its drawing) on a world of about --lines table lines of which about
--listed are in the novel list (tests/predict_report_cases.timing_world).  Both routes start with the novel list, the screened
table and `_cluster.txt` on disk and end with `_corrected.tsv`, the report and the profile file closed:

  (a) the rule in Python over the same three files (tests/predict_report_model.standin: strings, lists and dicts, the
      reference's own `list.remove` loop included);
  (b) predict.report_candidates: the native reader, Engine.predict_report (upload, the three device calls, download) and the
      native writers, each timed.

After one warm-up of each, the two routes alternate --runs times in this one process.  The three files of the two routes must
be equal.  No ratio is fixed in advance.  Writes one JSON object to --json, default profiles/predict_report_timing.json, and
prints it."""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def spread(xs):
    return dict(min=round(min(xs), 6), max=round(max(xs), 6))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lines", type=int, default=10_000)
    ap.add_argument("--listed", type=int, default=2_000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "predict_report_timing.json"))
    args = ap.parse_args()
    from mirge_amd import predict
    from mirge_amd.engine import Engine
    from tests import predict_report_cases as cases
    from tests import predict_report_model as rule
    texts = cases.timing_world(args.lines, args.listed)
    res = dict(what="predict mode: the report from the novel list, the screened table and the cluster file", lines=texts[1].count("\n") - 1,
               listed=texts[0].count("\n") - 1, runs=args.runs, input_bytes=sum(len(t) for t in texts))
    eng = Engine(0)
    try:
        with tempfile.TemporaryDirectory() as d:
            paths = [os.path.join(d, nm) for nm in (cases.NOVEL, cases.TABLE, cases.CLUSTER)]
            for p, text in zip(paths, texts):
                with open(p, "w") as fh:
                    fh.write(text)
            out = predict.report_paths(*paths)
            laps_a, laps_b, parts, kept = [], [], [], {}
            for k in range(args.runs + 1):
                t0 = time.perf_counter()
                entries = rule.standin(*paths)
                t1 = time.perf_counter()
                if k:
                    laps_a.append(t1 - t0)
                for key, p in out.items():
                    with open(p) as fh:
                        kept[key] = fh.read()
                    os.remove(p)
                timings = {}
                t0 = time.perf_counter()
                got = predict.report_candidates(eng, dict(novel=paths[0], table=paths[1], cluster=paths[2]), timings=timings)
                t1 = time.perf_counter()
                if k:
                    laps_b.append(t1 - t0)
                    parts.append(timings)
                assert got["entries"] == entries
                for key, p in out.items():
                    with open(p) as fh:
                        assert fh.read() == kept[key], key
                    os.remove(p)
            res.update(entries=entries, read_rows=int(got["row_off"][-1]), host_lines=got["host_lines"], host_entries=got["host_entries"],
                       output_bytes=sum(len(v) for v in kept.values()), files_equal=True)
            res["a_rule_s"] = spread(laps_a)
            res["b_array_route_s"] = spread(laps_b)
            res["b_split_s"] = {key: spread([p[key] for p in parts]) for key in ("read_s", "device_s", "write_s")}
            best = min(range(len(laps_b)), key=lambda i: laps_b[i])
            res["b_shares_of_the_fastest_run"] = {key: round(parts[best][key] / laps_b[best], 4) for key in ("read_s", "device_s", "write_s")}
    finally:
        eng.close()
    res["ratio_b_over_a"] = round(res["b_array_route_s"]["min"] / res["a_rule_s"]["min"], 5)
    res["command"] = "python scripts/predict_report_timing.py --lines %d --listed %d --runs %d" % (args.lines, args.listed, args.runs)
    os.makedirs(os.path.dirname(args.json), exist_ok=True)
    with open(args.json, "w") as fh:
        json.dump(res, fh)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
