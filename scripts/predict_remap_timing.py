#!/usr/bin/env python3
"""Timing of predict mode's second mapping (miRge2.0.py:566-601) on the world of scripts/predict_cluster_timing.py (a seeded
synthetic genome of --parts parts of --part-bases bases, --reads collapsed reads in piles), both laps starting at the return
of the trim writer, i.e. with `*_clusters_trimmed_orig.fa` on disk and the reads and the trim's arrays where that stage left
them:

  (a) the host route: mirge_amd.bowtie.align twice through files (the cluster FASTA as index, SAM text out, the second
      pass over the FASTA of the reads the first left unaligned), a Python restatement of the four functions of
      utils/processSam.py over those files (sets and dicts where the reference scans lists) and `LC_ALL=C sort -k6,6 -k1,1`;
  (b) the array route: predict.map_reads_to_clusters -- the library built on the device from the same FASTA, the two
      listings, mrg_predict_trim_reads / mrg_predict_remap_rows, the download and the native writer.

Both routes run --runs times in this one process; the files of the two routes must be equal.  No ratio is fixed in advance.
Writes one JSON object to --json, default profiles/predict_remap_timing.json, and prints it."""
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


def spread(xs):
    return dict(min=round(min(xs), 6), max=round(max(xs), 6))


def fasta_records(path):
    name, out = None, []
    with open(path) as fh:
        for line in fh:
            line = line.strip()
            if line.startswith(">"):
                name = line[1:].split()[0]
            elif line and name is not None:
                out.append((name, line))
                name = None
    return out


def host_route(reads_fa, orig_fa, stem, seed_length):
    """Route (a): every file the reference writes on its way, under `stem`."""
    from mirge_amd import bowtie
    ix = orig_fa[:-3]
    argv1 = [ix, reads_fa, "-f", "-n", "0", "-l", str(seed_length), "-S", "-a", "--best", "--norc", stem + "_tmp1.sam"]
    bowtie.align(bowtie.parse_align(argv1), "bowtie " + " ".join(argv1))
    # split_fasta_from_sam
    aligned = set()
    with open(stem + "_tmp1.sam") as fh:
        for line in fh:
            if line[0] != "@":
                f = line.split("\t", 2)
                if f[1] in ("0", "16"):
                    aligned.add(f[0])
    reads = fasta_records(reads_fa)
    left = reads_fa[:-3] + "_imperfectMath2Cluster.fa"
    with open(left, "w") as fh:
        fh.write("".join(">%s\n%s\n" % r for r in reads if r[0] not in aligned))
    argv2 = [ix, left, "-f", "-n", "1", "-l", "15", "-5", "1", "-3", "3", "-S", "-a", "--best", "--strata", "--norc", stem + "_tmp2.sam"]
    bowtie.align(bowtie.parse_align(argv2), "bowtie " + " ".join(argv2))
    # combineSam
    with open(stem + ".sam", "w") as out:
        with open(stem + "_tmp1.sam") as fh:
            for line in fh:
                if line[0] == "@" or line.split("\t", 2)[1] in ("0", "16"):
                    out.write(line)
        with open(stem + "_tmp2.sam") as fh:
            for line in fh:
                if line[0] != "@":
                    out.write(line)
    # decorateSam
    seq_of, cluster_of = dict(reads), dict(fasta_records(orig_fa))
    with open(stem + "_modified.sam", "w") as out, open(stem + ".sam") as fh:
        for line in fh:
            if line[0] == "@":
                out.write(line)
                continue
            f = line.strip().split("\t")
            out.write("\t".join([f[0], f[0].split("_")[-1], seq_of[f[0]], cluster_of.get(f[2], "*")] + f[1:]) + "\n")
    # parse_refine_sam (with --norc the reverseKept file equals the selected one; the reference writes both)
    with open(stem + "_modified_selected.tsv", "w") as o1, open(stem + "_modified_selected_reverseKept.tsv", "w") as o2, \
            open(stem + "_modified.sam") as fh:
        for line in fh:
            if line[0] != "@":
                flag = line.split("\t", 5)[4]
                if flag in ("0", "256"):
                    o1.write(line)
                    o2.write(line)
                elif flag in ("16", "272"):
                    o2.write(line)
    with open(stem + "_modified_selected_sorted.tsv", "w") as out:
        subprocess.run(["sort", "-k6,6", "-k1,1", stem + "_modified_selected.tsv"], stdout=out, check=True, env=dict(os.environ, LC_ALL="C"))
    return stem + "_modified_selected_sorted.tsv"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", type=int, default=3)
    ap.add_argument("--part-bases", type=int, default=100_000_000)
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--cutoff", type=int, default=30)
    ap.add_argument("--seed-length", type=int, default=25)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "predict_remap_timing.json"))
    args = ap.parse_args()
    import predict_cluster_timing as world
    from mirge_amd import predict
    from mirge_amd.engine import STRATUM_ALL
    with tempfile.TemporaryDirectory() as d:
        t0 = time.time()
        world.synthesize(d, args.parts, args.part_bases, args.reads)
        res = dict(what="predict mode: reads mapped back to the trimmed clusters", parts=args.parts, part_bases=args.part_bases,
                   reads=args.reads, cutoff=args.cutoff, seed_length=args.seed_length, runs=args.runs,
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
        orig_fa = out_stem + "_vs_genome_sorted_clusters_trimmed_orig.fa"
        res["clusters"], res["retained"], res["orig_fa_bytes"] = len(cl["entry"]), tr["n_retained"], os.path.getsize(orig_fa)
        # (b) first: the first call pays the kernels' first use, so one call ahead of the laps
        predict.map_reads_to_clusters(eng, rs, numbers, counts, tr, args.seed_length, out_stem)
        laps = []
        for _ in range(args.runs):
            tm = {}
            t = time.perf_counter()
            got = predict.map_reads_to_clusters(eng, rs, numbers, counts, tr, args.seed_length, out_stem, timings=tm)
            laps.append(dict(total_s=time.perf_counter() - t, device_ms=tm["list_ms"] + tm["rows_ms"], rows_ms=tm["rows_ms"],
                             download_ms=tm["download_ms"], write_s=tm["write_s"]))
        res["b_array_route"] = {k: spread([lap[k] for lap in laps]) for k in laps[0]}
        res["b_writer_share"] = spread([lap["write_s"] / lap["total_s"] for lap in laps])
        res.update(rows=got["n_rows"], aligned_pass1=got["aligned1"], aligned_pass2=got["aligned2"], unaligned=got["unaligned"])
        table_b = open(out_stem + predict.REMAP_SUFFIX, "rb").read()
        res["table_bytes"] = len(table_b)
        eng.close()
        # (a) the host route through files
        reads_fa = os.path.join(d, "reads.fa")
        stem_a = os.path.join(d, "a_vs_representative_seq")
        laps = []
        for _ in range(args.runs):
            t = time.perf_counter()
            path_a = host_route(reads_fa, orig_fa, stem_a, args.seed_length)
            laps.append(time.perf_counter() - t)
        res["a_host_route_s"] = spread(laps)
        res["files_equal"] = open(path_a, "rb").read() == table_b
        assert res["files_equal"], "the two routes' files differ"
    a, b = res["a_host_route_s"], res["b_array_route"]["total_s"]
    res["ratio_b_over_a"] = dict(best=round(b["min"] / a["max"], 5), worst=round(b["max"] / a["min"], 5))
    res["command"] = "python scripts/predict_remap_timing.py --parts %d --part-bases %d --reads %d" % (args.parts, args.part_bases, args.reads)
    text = json.dumps(res)
    with open(args.json, "w") as fh:
        fh.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
