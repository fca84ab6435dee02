#!/usr/bin/env python3
"""Timing of predict mode's precursor candidates (miRge2.0.py:608) on the world scripts/predict_features_timing.py makes
(the world of scripts/predict_cluster_timing.py with the read piles deepened, so that clusters pass the feature stage's
filter in number).  Both laps start at the return of predict.cluster_features, i.e. with `*_sorted_features.tsv` on disk and
the groups, frames and retained clusters where that stage left them on the device, and end with `*_features_precusor.fa`
closed:

  (a) the Python model over the feature file's text (tests/predict_precursors_model.run: a slice, a translate and a replace
      per window; seen names in a set -- the reference's own loop asks a LIST, quadratic in the lines, and builds a Biopython
      Seq per window, so it is slower still);
  (b) predict.cluster_precursors: mrg_predict_precursors, mrg_predict_precursor_bases, the download and the native writer.

Each route runs once as a warm-up and then --runs times in this one process; the files of the two routes must be equal.  No
ratio is fixed in advance.  Writes one JSON object to --json, default profiles/predict_precursors_timing.json, and prints
it."""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402


def spread(xs):
    return dict(min=round(min(xs), 6), max=round(max(xs), 6))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", type=int, default=2)
    ap.add_argument("--part-bases", type=int, default=20_000_000)
    ap.add_argument("--reads", type=int, default=120_000)
    ap.add_argument("--reads-per-locus", type=int, default=10)
    ap.add_argument("--deep", type=int, default=8_000)
    ap.add_argument("--cutoff", type=int, default=30)
    ap.add_argument("--seed-length", type=int, default=25)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "predict_precursors_timing.json"))
    args = ap.parse_args()
    import predict_cluster_timing as world
    import predict_features_timing as features_world
    from mirge_amd import predict
    from mirge_amd.engine import STRATUM_ALL
    from tests import predict_precursors_model as model
    with tempfile.TemporaryDirectory() as d:
        t0 = time.time()
        chromosomes = features_world.synthesize(d, args.parts, args.part_bases, args.reads, args.reads_per_locus, args.deep)
        res = dict(what="predict mode: the precursor candidates", parts=args.parts, part_bases=args.part_bases, reads=args.reads,
                   reads_per_locus=args.reads_per_locus, deep=args.deep, cutoff=args.cutoff, seed_length=args.seed_length, runs=args.runs,
                   synthesis_and_index_build_s=round(time.time() - t0, 1))
        eng, parts, keys, names, seqs, rs = world.open_world(d)
        counts = predict.read_counts(names)
        numbers = predict.read_numbers(names)
        keep = np.array(["chr" in nm for ix in parts for nm in ix.names], dtype=bool)
        cl = eng.cluster_valid(rs, keys, counts, entry_keep=keep, threshold=14, strands=2, stratum_mode=STRATUM_ALL, m=3, seed_len=25,
                               max_mm_seed=0, max_mm_total=2, keep_device=True)
        out_stem = os.path.join(d, "unmapped_mirna_smp")
        predict.write_clusters(out_stem + "_vs_genome_sorted_clusters.tsv", predict.sample_name(out_stem + "_vs_genome_sorted.sam"), parts,
                               names, cl)
        tr = predict.trim_clusters(eng, cl, predict.load_repeats(None, parts), args.cutoff, out_stem, names)
        tr = dict(tr, clusters=predict.retained_clusters(cl, tr))
        remap = predict.map_reads_to_clusters(eng, rs, numbers, counts, tr, args.seed_length, out_stem, keep_device=True)
        t = time.perf_counter()
        feats = predict.cluster_features(eng, rs, counts, tr, remap, parts, out_stem, keep_device=True)
        res.update(clusters=len(cl["entry"]), retained=tr["n_retained"], rows=remap["n_rows"], groups=feats["seen"],
                   feature_lines=feats["lines"], feature_stage_s=round(time.perf_counter() - t, 3))
        features_path = out_stem + predict.REMAP_SUFFIX[:-4] + predict.FEATURES_SUFFIX
        fasta_path = out_stem + predict.REMAP_SUFFIX[:-4] + predict.PRECURSOR_SUFFIX
        res["features_bytes"] = os.path.getsize(features_path)
        # (b): one call ahead of the laps pays the kernels' first use and the libraries' segment tables
        laps = []
        for k in range(args.runs + 1):
            tm = {}
            t = time.perf_counter()
            got = predict.cluster_precursors(eng, feats, tr, parts, out_stem, timings=tm, parts_libs=keys)
            total = time.perf_counter() - t
            print("# route b, lap %d: %.4f s" % (k, total), file=sys.stderr, flush=True)
            if k:
                laps.append(dict(total_s=total, device_ms=tm["device_ms"], download_ms=tm["download_ms"], write_s=tm["write_s"]))
        res["b_array_route"] = {k: spread([lap[k] for lap in laps]) for k in laps[0]}
        res["b_writer_share"] = spread([lap["write_s"] / lap["total_s"] for lap in laps])
        res["b_device_share"] = spread([lap["device_ms"] / 1000.0 / lap["total_s"] for lap in laps])
        res.update(records=got["records"], fasta_bytes=got["bytes"], sequence_bytes=len(got["seq"]))
        file_b = open(fasta_path, "rb").read()
        eng.close()
        # (a) the model over the feature file's text
        laps = []
        for k in range(args.runs + 1):
            t = time.perf_counter()
            text = model.run(open(features_path).read(), chromosomes)
            with open(os.path.join(d, "a" + predict.PRECURSOR_SUFFIX), "w") as fh:
                fh.write(text)
            print("# route a, lap %d: %.3f s" % (k, time.perf_counter() - t), file=sys.stderr, flush=True)
            if k:
                laps.append(time.perf_counter() - t)
        res["a_model_route_s"] = spread(laps)
        res["files_equal"] = text.encode() == file_b
        assert res["files_equal"], "the two routes' files differ"
    a, b = res["a_model_route_s"], res["b_array_route"]["total_s"]
    res["ratio_b_over_a"] = dict(best=round(b["min"] / a["max"], 5), worst=round(b["max"] / a["min"], 5))
    res["command"] = "python scripts/predict_precursors_timing.py --parts %d --part-bases %d --reads %d --reads-per-locus %d --deep %d" % (
        args.parts, args.part_bases, args.reads, args.reads_per_locus, args.deep)
    out = json.dumps(res)
    with open(args.json, "w") as fh:
        fh.write(out + "\n")
    print(out)


if __name__ == "__main__":
    main()
