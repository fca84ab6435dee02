#!/usr/bin/env python3
"""Timing of `annotate -trf`'s tRFs.samples.tmp/ stage on the world of scripts/trf_tables_timing.py (--reads distinct tRNA
reads on --trnas mature tRNAs and as many trailers, --samples samples): from the return of columnar.write_trf_tables to the
last file of tRFs.samples.tmp/, --runs runs of each route, alternating, after one warm-up of the array route:

  (a) the parent's route: pack.unpack_reads + trf.content_from_rows + trf_samples.write_trf_samples (Engine.trf_peaks);
  (b) the array route: trf.sample_tables + trf_samples.write_trf_samples_arrays (Engine.trf_sample_groups on the
      device-resident arrays a cascade leaves behind, mrg_write_trf_sample_reports, Engine.trf_peaks_groups, mrg_trf_rank).

Host clocks around each route and, for (b), around its stages (`groups_s` the two mrg_trf_sample_groups calls and the
download, `reports_s` the native writer, `peaks_s` the three density-peak passes with the rank and the label pass in Python,
`clusters_s` .clusters.detail and .tRFs.report.tsv in Python); device events around the counting and the filling call and,
inside the filling call, around its four stages.  Every file of tRFs.samples.tmp/ is compared byte for byte between the
routes.  Writes one JSON object to --json (default profiles/trf_samples_timing.json) and prints it; `passed` = equal files
and the slowest run of (b) not slower than the fastest run of (a).  --labels: see labels_leg (writes
profiles/trf_samples_timing_labels.json).  Needs a GPU."""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import numpy as np  # noqa: E402


def parent_route(w, et, t_rec, eng, outdir, sample_list, denom):
    from mirge_amd import pack, trf, trf_samples
    t0 = time.time()
    idx = t_rec[:, 0]
    seqs = pack.unpack_reads(np.ascontiguousarray(w["words"][:, idx]), w["lens"][idx], None)
    content = trf.content_from_rows(et, t_rec, seqs, w["quant"][idx], denom)
    t1 = time.time()
    trf_samples.write_trf_samples(outdir, sample_list, content, w["tables"], w["pre"], trf_samples.engine_peaks(eng))
    t2 = time.time()
    return dict(content_from_rows_s=t1 - t0, write_trf_samples_s=t2 - t1, total_s=t2 - t0)


def array_route(w, dev, et, t_rec, eng, outdir, sample_list, denom, device_labels=False):
    import torch
    from mirge_amd import trf, trf_samples
    torch.cuda.synchronize()
    t0 = time.time()
    st = trf.sample_tables(et, w["tables"], w["pre"])
    t1 = time.time()
    timings = {}
    trf_samples.write_trf_samples_arrays(outdir, sample_list, et, st, t_rec, w["words"], w["lens"], None, w["quant"], denom,
                                         w["tables"], w["pre"], trf_samples.engine_groups(eng, dev),
                                         trf_samples.engine_peaks_groups(eng), timings=timings, device_rank=True,
                                         device_labels=device_labels)
    t2 = time.time()
    return dict(sample_tables_s=t1 - t0, total_s=t2 - t0, **{k: float(v) for k, v in timings.items()})


def labels_leg(args, w, on_device, et, t_rec, eng, d, sample_list, denom):
    """--labels: the array route with the label pass and the two cluster files in Python (device_labels=False, the parent's)
    against the same route with mrg_trf_assign / mrg_trf_halo / mrg_write_trf_cluster_reports (device_labels=True): --runs
    runs of each, alternating, after a warm-up of both; `peaks_s + clusters_s` of every run, the medians, device events around
    the new calls, and all files compared byte for byte.  The world's reads are random and its RP100K small: as it is, no group
    has a cluster (`clusters` = 0); --denom-div raises the RP100K of both routes alike until there are."""
    import torch
    from mirge_amd import trf, trf_samples
    dirs = {False: os.path.join(d, "labels_off"), True: os.path.join(d, "labels_on")}
    for flag in (False, True):
        os.mkdir(dirs[flag])
        array_route(w, on_device, et, t_rec, eng, dirs[flag], sample_list, denom, flag)      # warm-up
    out = dict(what="annotate -trf: peaks_s + clusters_s of the array route, labels and cluster files in Python (parent) or from "
                    "the arrays (device_labels)", reads=args.reads, trnas=args.trnas, samples=args.samples, denom_div=args.denom_div, parent=[], device_labels=[],
               command="python scripts/trf_samples_timing.py " + " ".join(sys.argv[1:]))
    for run in range(args.runs):
        for flag, key in ((False, "parent"), (True, "device_labels")):
            r = array_route(w, on_device, et, t_rec, eng, dirs[flag], sample_list, denom, flag)
            r["peaks_plus_clusters_s"] = r["peaks_s"] + r["clusters_s"]
            out[key].append(r)
            print("run %d %s: peaks %.3f s + clusters %.3f s" % (run, key, r["peaks_s"], r["clusters_s"]), flush=True)
    ta, tb = (os.path.join(dirs[f], "tRFs.samples.tmp") for f in (False, True))
    names = sorted(os.listdir(ta))
    same = names == sorted(os.listdir(tb)) and len(names) == 4 * args.samples
    for fn in names:
        same = same and open(os.path.join(ta, fn), "rb").read() == open(os.path.join(tb, fn), "rb").read()
    assert same, "the files of the two routes differ"
    # the new device calls alone, between events
    g = eng.trf_sample_groups(trf.sample_tables(et, w["tables"], w["pre"]), t_rec, *on_device, denom)
    state = eng.trf_peaks_groups(g, trf_samples.gaussian_table())
    state.rank()
    state.min_distance(None)
    ms = {}

    def timed(key, fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        res = fn()
        e1.record()
        e1.synchronize()
        ms.setdefault(key, []).append(e0.elapsed_time(e1))
        return res
    for _ in range(args.runs + 1):
        nclust = timed("assign_ms", state.assign)[0]
        bord_off = np.zeros(len(nclust) + 1, dtype=np.uint32)
        bord_off[1:] = np.cumsum(np.where(nclust > 1, nclust.astype(np.uint64) + 1, 0))
        timed("border_ms", lambda: state.border(None, bord_off))
        timed("halo_ms", lambda: state.halo())
    med = lambda v: float(np.median(v))
    out.update(files_equal=bool(same), groups=int(g.G), rows=int(g.n), clusters=int(len(state.centers)),
               device_calls_ms={k: [round(x, 3) for x in v[1:]] for k, v in ms.items()},
               parent_median_s=med([r["peaks_plus_clusters_s"] for r in out["parent"]]),
               device_labels_median_s=med([r["peaks_plus_clusters_s"] for r in out["device_labels"]]))
    out["passed"] = bool(same and out["device_labels_median_s"] < out["parent_median_s"])
    text = json.dumps(out)
    with open(args.json, "w") as fh:
        fh.write(text + "\n")
    print(text)
    return 0 if out["passed"] else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1000000)
    ap.add_argument("--trnas", type=int, default=4000)
    ap.add_argument("--samples", type=int, default=2)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--labels", action="store_true", help="time the label pass and the cluster files: Python against the arrays")
    ap.add_argument("--denom-div", type=int, default=1, help="with --labels: divide the RP100K denominators, so that the random "
                    "reads of the world reach the density of cluster centres (rho >= 5); 1 = the world as it is, without cluster")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if args.json is None:
        args.json = os.path.join(ROOT, "profiles", "trf_samples_timing_labels.json" if args.labels else "trf_samples_timing.json")
    import torch
    from trf_tables_timing import synthesize
    from mirge_amd import columnar, trf
    from mirge_amd.engine import Engine
    from mirge_amd.index import FmIndex
    eng = Engine(0)          # (raises without a GPU)
    t0 = time.time()
    w = synthesize(args.trnas, args.reads, args.samples)
    for key in ("mature_trna", "pre_trna"):
        eng.add_library(key, FmIndex.build(*w["libs"][key]))
    print("synthesised %d reads on %d tRNAs in %.1f s" % (args.reads, args.trnas, time.time() - t0), flush=True)
    dev = {k: torch.from_numpy(w[k].view(np.int64) if k == "words" else w[k].view(np.int32) if k == "quant" else w[k]).to(eng.device)
           for k in ("words", "lens", "pass_id", "quant")}
    sample_list = ["s%d.fastq" % i for i in range(args.samples)]
    denom = [q["maturetrnaReads"] + q["pretrnaReads"] for q in w["log_dic"]["quantStats"]]
    out = dict(what="annotate -trf: tRFs.samples.tmp/ from the return of columnar.write_trf_tables to its last file", reads=args.reads,
               trnas=args.trnas, samples=args.samples, parent_route=[], array_route=[],
               command="python scripts/trf_samples_timing.py " + " ".join(sys.argv[1:]))
    with tempfile.TemporaryDirectory() as d:
        a_dir, b_dir = os.path.join(d, "a"), os.path.join(d, "b")
        os.mkdir(a_dir)
        os.mkdir(b_dir)
        et = trf.entry_tables(w["libs"]["mature_trna"][0], w["libs"]["pre_trna"][0], w["tables"], w["pre"])
        rec, hits, n2, _ = eng.trf_classify(et, dev["words"], dev["lens"], None, dev["pass_id"])
        t_rec, _ = columnar.write_trf_tables(d, sample_list, w["log_dic"], w["words"], w["lens"], None, w["quant"], rec, hits, n2, et)
        on_device = (dev["words"], dev["lens"], None, dev["quant"])
        if args.labels:
            denom = [max(1, x // args.denom_div) for x in denom]
            return labels_leg(args, w, on_device, et, t_rec, eng, d, sample_list, denom)
        array_route(w, on_device, et, t_rec, eng, b_dir, sample_list, denom)    # warm-up: code objects
        print("warm-up done", flush=True)
        for run in range(args.runs):
            r = parent_route(w, et, t_rec, eng, a_dir, sample_list, denom)
            out["parent_route"].append(r)
            print("run %d parent route %.2f s" % (run, r["total_s"]), flush=True)
            r = array_route(w, on_device, et, t_rec, eng, b_dir, sample_list, denom)
            out["array_route"].append(r)
            print("run %d array route %.2f s" % (run, r["total_s"]), flush=True)
            with open(args.json, "w") as fh:          # (what has been measured so far survives an interrupted run)
                fh.write(json.dumps(out) + "\n")
        ta, tb = os.path.join(a_dir, "tRFs.samples.tmp"), os.path.join(b_dir, "tRFs.samples.tmp")
        names = sorted(os.listdir(ta))
        same = names == sorted(os.listdir(tb)) and len(names) == 4 * args.samples
        for fn in names:
            same = same and open(os.path.join(ta, fn), "rb").read() == open(os.path.join(tb, fn), "rb").read()
        out["file_bytes"] = {fn: os.path.getsize(os.path.join(tb, fn)) for fn in sorted(os.listdir(tb))}
    assert same, "the files of the two routes differ"
    old = [r["total_s"] for r in out["parent_route"]]
    new = [r["total_s"] for r in out["array_route"]]
    out["files_equal"] = bool(same)
    out["parent_fastest_s"], out["array_slowest_s"] = min(old), max(new)
    out["ratio_parent_fastest_over_array_slowest"] = round(min(old) / max(new), 2)
    out["passed"] = bool(same and max(new) <= min(old))
    text = json.dumps(out)
    with open(args.json, "w") as fh:
        fh.write(text + "\n")
    print(text)
    return 0 if out["passed"] else 1


if __name__ == "__main__":
    sys.exit(main())
