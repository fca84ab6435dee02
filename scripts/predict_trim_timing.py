#!/usr/bin/env python3
"""Timing of predict mode's preliminary trim (miRge2.0.py:557-562) on the world of scripts/predict_cluster_timing.py (a seeded
synthetic genome of --parts parts of --part-bases bases, --reads collapsed reads in piles) and a synthetic repeat table of
--elements elements (random starts on every part, 20-300 bases long, 1000 family names):

  (a) tests/predict_trim_model.py over the written `*_clusters.tsv`, standing in for the loops of preTrimClusteredSeq.py and
      generate_Seq.py (Biopython is not needed by the model; the reference itself reads the table back the same way, one
      line at a time, and builds sets of every coordinate where the model compares interval ends);
  (b) the array route: predict.trim_clusters from the return value of Engine.cluster_valid(keep_device=True) to the last byte
      of the three files -- the device lap (mrg_predict_trim) and the downloads between events, the writer by the clock.

Both routes run --runs times in this one process; the files of the two routes must be equal.  Loading the repeat table
(load_repeats / flat_repeats) is outside both laps, as unpickling is outside the reference's loop.  Writes one JSON object
to --json, default profiles/predict_trim_timing.json, and prints it."""
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


def write_repeats(path, parts, part_bases, n):
    rng = np.random.default_rng(557)
    part = rng.integers(0, parts, n)
    start = rng.integers(1, part_bases, n)
    end = start + rng.integers(19, 300, n)
    fam = rng.integers(0, 1000, n)
    with open(path, "w") as fh:
        fh.write("".join("chr%d\t%d\t%d\tfam%d\n" % (p + 1, s, e, f) for p, s, e, f in zip(part.tolist(), start.tolist(), end.tolist(),
                                                                                         fam.tolist())))


def spread(xs):
    return dict(min=round(min(xs), 6), max=round(max(xs), 6))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", type=int, default=3)
    ap.add_argument("--part-bases", type=int, default=100_000_000)
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--elements", type=int, default=1_000_000)
    ap.add_argument("--cutoff", type=int, default=30)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "predict_trim_timing.json"))
    args = ap.parse_args()
    import predict_cluster_timing as world
    from mirge_amd import predict
    from mirge_amd.engine import STRATUM_ALL
    from tests import predict_trim_model as model
    with tempfile.TemporaryDirectory() as d:
        t0 = time.time()
        world.synthesize(d, args.parts, args.part_bases, args.reads)
        rep_path = os.path.join(d, "g_repeats.tsv")
        write_repeats(rep_path, args.parts, args.part_bases, args.elements)
        res = dict(what="predict mode: preliminary trim of the location clusters", parts=args.parts, part_bases=args.part_bases,
                   reads=args.reads, elements=args.elements, cutoff=args.cutoff, runs=args.runs,
                   synthesis_and_index_build_s=round(time.time() - t0, 1))
        eng, parts, keys, names, seqs, rs = world.open_world(d)
        t = time.time()
        repeats = predict.load_repeats(rep_path, parts)
        res["load_repeats_s"] = round(time.time() - t, 3)
        counts = predict.read_counts(names)
        keep = np.array(["chr" in nm for ix in parts for nm in ix.names], dtype=bool)
        cl = eng.cluster_valid(rs, keys, counts, entry_keep=keep, threshold=14, strands=2, stratum_mode=STRATUM_ALL, m=3, seed_len=25,
                               max_mm_seed=0, max_mm_total=2, keep_device=True)
        stem_b = os.path.join(d, "smp_x_y")
        table = stem_b + "_vs_genome_sorted_clusters.tsv"
        predict.write_clusters(table, predict.sample_name(stem_b + "_vs_genome_sorted.sam"), parts, names, cl)
        res["clusters"], res["table_bytes"] = len(cl["entry"]), os.path.getsize(table)
        # (b) first: the first call pays the kernels' first use, so one call ahead of the laps
        predict.trim_clusters(eng, cl, repeats, args.cutoff, stem_b, names)
        laps = []
        for _ in range(args.runs):
            tm = {}
            t = time.perf_counter()
            tr = predict.trim_clusters(eng, cl, repeats, args.cutoff, stem_b, names, timings=tm)
            laps.append(dict(total_s=time.perf_counter() - t, trim_ms=tm["trim_ms"], download_ms=tm["download_ms"], write_s=tm["write_s"]))
        res["b_array_route"] = {k: spread([lap[k] for lap in laps]) for k in laps[0]}
        res["retained"] = tr["n_retained"]
        got = [open(table[:-4] + sfx, "rb").read() for sfx in ("_trimmed.tsv", "_trimmed.fa", "_trimmed_orig.fa")]
        res["trimmed_bytes"] = [len(x) for x in got]
        eng.close()
        # (a) the sequential model over the table's text
        entries = [nm for ix in parts for nm in ix.names]
        flat = (repeats["rep_off"].tolist(), repeats["start"].tolist(), repeats["end"].tolist(), repeats["name_id"].tolist(),
                repeats["names"])
        laps = []
        for _ in range(args.runs):
            t = time.perf_counter()
            with open(table) as fh:
                want = model.files_flat(fh.read(), entries, flat, args.cutoff)
            for sfx, text in zip(("_a.tsv", "_a.fa", "_a_orig.fa"), want):
                with open(table[:-4] + sfx, "w") as fh:
                    fh.write(text)
            laps.append(time.perf_counter() - t)
        res["a_sequential_model_s"] = spread(laps)
        res["files_equal"] = [w.encode() == g for w, g in zip(want, got)]
        for w, g in zip(want, got):
            if w.encode() != g:
                a_lines, b_lines = w.split("\n"), g.decode().split("\n")
                k = next((i for i, (x, y) in enumerate(zip(a_lines, b_lines)) if x != y), min(len(a_lines), len(b_lines)))
                sys.stderr.write("line %d differs:\n(a) %s\n(b) %s\n" % (k + 1, a_lines[k:k + 1], b_lines[k:k + 1]))
        assert all(res["files_equal"]), "the two routes' files differ"
    a, b = res["a_sequential_model_s"], res["b_array_route"]["total_s"]
    res["ratio_b_over_a"] = dict(best=round(b["min"] / a["max"], 5), worst=round(b["max"] / a["min"], 5))
    res["command"] = "python scripts/predict_trim_timing.py --parts %d --part-bases %d --reads %d --elements %d" % (
        args.parts, args.part_bases, args.reads, args.elements)
    text = json.dumps(res)
    with open(args.json, "w") as fh:
        fh.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
