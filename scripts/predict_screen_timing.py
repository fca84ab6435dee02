#!/usr/bin/env python3
"""Timing of predict mode's screening of the folded candidates (miRge2.0.py:610-626) on the world
scripts/predict_precursors_timing.py runs on, with tests/fold_standin.py as the folder on both sides.  A Python process per
candidate (about 0.12 s each) cannot finish a full table, so both routes are timed on the first --lines feature lines (cut
back to a line that needs no neighbour behind the cut); the JSON states the lines timed and their fraction of the table.  Both
start with `*_features_precusor.str` on disk (the first fold is common to both and timed once, as fold1_s) and end with
`*_features_updated_stableClusterSeq_15.tsv` closed:

  (a) the reference-shaped route: tests/predict_screen_model.py over the texts, one fold PROCESS per candidate as the
      reference's os.system call, a line-at-a-time writer;
  (b) predict.screen_precursors: the native reader, the four device calls, ONE fold process over all pruned candidates, the
      host path's share and the native writer, each reported.

The two files must be equal.  No ratio is fixed in advance.  Writes one JSON object to --json and prints it."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", type=int, default=2)
    ap.add_argument("--part-bases", type=int, default=20_000_000)
    ap.add_argument("--reads", type=int, default=120_000)
    ap.add_argument("--reads-per-locus", type=int, default=10)
    ap.add_argument("--deep", type=int, default=8_000)
    ap.add_argument("--cutoff", type=int, default=30)
    ap.add_argument("--seed-length", type=int, default=25)
    ap.add_argument("--lines", type=int, default=300)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "predict_screen_timing.json"))
    args = ap.parse_args()
    import predict_cluster_timing as world
    import predict_features_timing as features_world
    from mirge_amd import predict
    from mirge_amd.engine import STRATUM_ALL
    from tests import predict_screen_cases as cases
    from tests import predict_screen_model as model
    with tempfile.TemporaryDirectory() as d:
        t0 = time.time()
        features_world.synthesize(d, args.parts, args.part_bases, args.reads, args.reads_per_locus, args.deep)
        res = dict(what="predict mode: the screening of the folded candidates", parts=args.parts, part_bases=args.part_bases,
                   reads=args.reads, reads_per_locus=args.reads_per_locus, deep=args.deep, cutoff=args.cutoff, seed_length=args.seed_length,
                   folder="tests/fold_standin.py on both sides", synthesis_and_index_build_s=round(time.time() - t0, 1))
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
        feats = predict.cluster_features(eng, rs, counts, tr, remap, parts, out_stem, keep_device=True)
        prec = predict.cluster_precursors(eng, feats, tr, parts, out_stem, parts_libs=keys)
        table = out_stem + predict.REMAP_SUFFIX[:-4]
        features_path, fasta_path = table + predict.FEATURES_SUFFIX, table + predict.PRECURSOR_SUFFIX
        # the first lines of the table, cut back until the model finds every neighbour it needs
        text = open(features_path).read().splitlines(True)
        n = min(args.lines, len(text) - 1)
        while n > 0:
            try:
                model.candidates(model.read_features("".join(text[:n + 1]))[1])
                break
            except IndexError:
                n -= 1
        res.update(feature_lines=len(text) - 1, lines_timed=n, fraction_of_the_lines=round(n / max(len(text) - 1, 1), 5))
        with open(features_path, "w") as fh:
            fh.write("".join(text[:n + 1]))
        fasta = open(fasta_path).read().splitlines(True)
        with open(fasta_path, "w") as fh:
            fh.write("".join(fasta[:4 * n]))
        prec = dict(rec_group=prec["rec_group"][:2 * n], records=2 * n)
        # (b) one call ahead of the lap pays the kernels' first use; the folds are the stand-in's and dominate either way
        laps = []
        for k in range(2):
            tm = {}
            t = time.perf_counter()
            got = predict.screen_precursors(eng, feats, prec, cases.STANDIN, out_stem, timings=tm)
            tm["total_s"] = time.perf_counter() - t
            print("# route b, lap %d: %.3f s" % (k, tm["total_s"]), file=sys.stderr, flush=True)
            laps.append(tm)
        tm = laps[1]
        res["b_array_route"] = {k: round(float(v), 6) for k, v in tm.items()}
        res["b_after_fold1_s"] = round(tm["total_s"] - tm["fold1_s"], 6)
        res.update(candidates=got["candidates"], pruned_folded=got["pruned"], host_candidates=got["host_candidates"], fold_calls_b=got["folds"])
        file_b = open(got["path"], "rb").read()
        eng.close()
        # (a) from the same `.str`: the model, one fold process per candidate, a line at a time
        str_text = open(table + "_features_precusor.str").read()
        started = [0]

        def fold_each(sequences):
            out = []
            for s in sequences:
                done = subprocess.run([cases.STANDIN, "--noPS", "--noLP"], input=">c\n%s\n" % s, capture_output=True, text=True, check=True)
                started[0] += 1
                r = model.parse_str(done.stdout)[0]
                out.append((r[2], r[3]))
            return out
        t = time.perf_counter()
        header, lines = model.screen_lines(open(features_path).read(), str_text, fold_each, fold_each=True)
        with open(os.path.join(d, "a.tsv"), "w") as fh:
            fh.write(header.strip() + "\t" + model.HEADER_TAIL)
            for row in lines:
                best = row["best"]
                fh.write(row["line"].strip() + "\t" + (model.NONE_ROW if best is None else model.format_row(*row["candidates"][best])) + "\n")
        res["a_reference_shaped_route_s"] = round(time.perf_counter() - t, 3)
        res["fold_processes_a"] = started[0]
        res["files_equal"] = open(os.path.join(d, "a.tsv"), "rb").read() == file_b
        assert res["files_equal"], "the two routes' files differ"
    res["ratio_b_after_fold1_over_a"] = round(res["b_after_fold1_s"] / res["a_reference_shaped_route_s"], 5)
    res["command"] = "python scripts/predict_screen_timing.py --parts %d --part-bases %d --reads %d --reads-per-locus %d --deep %d --lines %d" % (
        args.parts, args.part_bases, args.reads, args.reads_per_locus, args.deep, args.lines)
    out = json.dumps(res)
    with open(args.json, "w") as fh:
        fh.write(out + "\n")
    print(out)


if __name__ == "__main__":
    main()
