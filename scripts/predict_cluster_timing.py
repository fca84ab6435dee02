#!/usr/bin/env python3
"""Timing of predict mode's map-and-cluster stage (miRge2.0.py:538-548) on a seeded synthetic genome of --parts parts of
--part-bases random bases (each its own library) and --reads collapsed reads of 16-25 nt, drawn in piles around loci so
that clusters form (80 % cut from the genome with 0-1 substitutions on either strand; the rest random):

  (a) the route before Engine.cluster_valid: the listing to the host (Engine.list_valid), the front end's SAM text
      (mrg_write_bowtie), a Python sort of its lines, and tests/predict_cluster_model.py standing in for the reference's
      Python loop (samtools is not used: its view / sort / index / view would come on top);
  (b) mirge_amd.predict.map_and_cluster's own steps: Engine.cluster_valid and mrg_write_clusters, without and with
      the sorted SAM file.

Every step runs in a child process of its own under --step-timeout seconds; the children share the index files the
parent builds.  Writes one JSON object (both routes, the device times of sort / scan / assemble, the row count, and
whether the two tables are equal) to --json, default profiles/predict_cluster_timing.json, and prints it."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def synthesize(d, parts, part_bases, n_reads):
    from mirge_amd.index import FmIndex
    rng = np.random.default_rng(538)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    texts = []
    for k in range(parts):
        t = acgt[rng.integers(0, 4, part_bases)].tobytes()
        texts.append(t)
        FmIndex.build(["chr%d" % (k + 1)], [t.decode()]).save(os.path.join(d, "g.part%03d.mrgfm" % k))
    loci = rng.integers(100, part_bases - 100, max(1, n_reads // 12))
    loci_p = rng.integers(0, parts, loci.size)
    comp = bytes.maketrans(b"ACGT", b"TGCA")
    seen, lines = set(), []
    while len(lines) < n_reads:
        L = int(rng.integers(16, 26))
        if rng.random() < 0.8:
            i = int(rng.integers(0, loci.size))
            at = int(loci[i]) + int(rng.integers(-30, 31))
            q = bytearray(texts[int(loci_p[i])][at:at + L])
            if rng.random() < 0.3:
                j = int(rng.integers(0, L))
                q[j] = b"ACGT"[(b"ACGT".index(q[j]) + 1) % 4]
            q = bytes(q)
            if rng.random() < 0.5:
                q = q[::-1].translate(comp)
        else:
            q = acgt[rng.integers(0, 4, L)].tobytes()
        if q not in seen:
            seen.add(q)
            lines.append(b">mir%d_%d\n%s\n" % (len(lines), 1 + len(lines) % 211, q))
    with open(os.path.join(d, "reads.fa"), "wb") as fh:
        fh.write(b"".join(lines))


def open_world(d):
    from mirge_amd import bowtie, pack
    from mirge_amd.engine import Engine, ReadSet
    eng = Engine(int(os.environ.get("MIRGE_AMD_GPU", "0")))
    parts = bowtie.open_index(os.path.join(d, "g"))
    keys = []
    for k, ix in enumerate(parts):
        keys.append("part%03d" % k)
        eng.add_library(keys[-1], ix, exact_dict=False)
    names, seqs = bowtie.read_fasta(os.path.join(d, "reads.fa"))
    words, lens, nmask = pack.pack_reads(seqs, 1)
    return eng, parts, keys, names, seqs, ReadSet(words, lens, nmask, device=eng.device)


def step_old(d):
    """Route (a)."""
    from mirge_amd import bowtie
    from mirge_amd.engine import STRATUM_ALL
    from tests import predict_cluster_model as model
    eng, parts, keys, names, seqs, rs = open_world(d)
    out = {}
    sam = os.path.join(d, "old_vs_genome.sam")
    for rep in ("first", "second"):      # the first call pays the allocator's and the kernels' first use
        tm = {}
        t = time.time()
        off, entry, offset, strand, mm, supp = eng.list_valid(rs, keys, strands=2, stratum_mode=STRATUM_ALL, m=3, seed_len=25,
                                                              max_mm_seed=0, max_mm_total=2, timings=tm)
        t_list = time.time() - t
        t = time.time()
        s = bowtie.write_bowtie(sam, True, "bowtie -f -n 0 -m 3 -l 25 -S -a --best genome reads.fa", parts, names, seqs, off,
                                entry, offset, strand, mm, supp, 3)
        out[rep] = dict(list_valid_s=t_list, sam_text_s=time.time() - t, count_sweeps_s=tm["count_s"], fill_sweeps_s=tm["fill_s"])
    out["sam_bytes"] = os.path.getsize(sam)
    out["alignments"] = s["reported"]
    eng.close()
    t = time.time()
    text = model.sort_sam(open(sam).read())
    out["python_sort_s"] = time.time() - t
    t = time.time()
    tsv = model.cluster_tsv(text, 14, "old")
    out["python_cluster_s"] = time.time() - t
    with open(os.path.join(d, "old_clusters.tsv"), "w") as fh:
        fh.write(tsv)
    out["total_s"] = out["second"]["list_valid_s"] + out["second"]["sam_text_s"] + out["python_sort_s"] + out["python_cluster_s"]
    return out


def step_new(d, sam):
    """Route (b): the steps of predict.map_and_cluster behind the reads and libraries being resident, as in (a)."""
    from mirge_amd import predict
    from mirge_amd.engine import STRATUM_ALL
    eng, parts, keys, names, seqs, rs = open_world(d)
    out = {}
    stem = os.path.join(d, "old_x_y")     # (sample name "old", as route (a) prints)
    for rep in ("first", "second"):      # the first call pays the allocator's and the kernels' first use
        tm = {}
        t = time.time()
        counts = predict.read_counts(names)
        keep = np.array(["chr" in nm for ix in parts for nm in ix.names], dtype=bool)
        cl = eng.cluster_valid(rs, keys, counts, entry_keep=keep, threshold=14, strands=2, stratum_mode=STRATUM_ALL, m=3,
                               seed_len=25, max_mm_seed=0, max_mm_total=2, sorted_rows=sam, timings=tm)
        t_cluster = time.time() - t
        t = time.time()
        predict.write_clusters(stem + "_vs_genome_sorted_clusters.tsv", "old", parts, names, cl)
        t_tsv = time.time() - t
        t_sam = 0.0
        if sam:
            t = time.time()
            predict.write_sorted_sam(stem + "_vs_genome_sorted.sam", parts, names, seqs, cl["rows"], cl["suppressed"], 3)
            t_sam = time.time() - t
        out[rep] = dict(cluster_valid_s=t_cluster, write_clusters_s=t_tsv, write_sorted_sam_s=t_sam,
                        total_s=t_cluster + t_tsv + t_sam, count_sweeps_s=tm["count_s"], fill_sweeps_s=tm["fill_s"],
                        sort_ms=tm.get("sort_ms"), scan_ms=tm.get("scan_ms"), assemble_ms=tm.get("assemble_ms"))
    out["rows"], out["rows_on_chr"], out["clusters"] = cl["n_rows"], cl["n_valid"], len(cl["entry"])
    eng.close()
    old = os.path.join(d, "old_clusters.tsv")
    if os.path.exists(old):
        out["table_equals_route_a"] = open(old).read() == open(stem + "_vs_genome_sorted_clusters.tsv").read()
    return out


def child(step, d, limit):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", step, "--dir", d], capture_output=True, text=True,
                       timeout=limit, cwd=ROOT)
    if r.returncode != 0:
        raise SystemExit("step %s failed (%d): %s" % (step, r.returncode, r.stderr[-2000:]))
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", type=int, default=3)
    ap.add_argument("--part-bases", type=int, default=100_000_000)
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--step-timeout", type=int, default=900)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "predict_cluster_timing.json"))
    ap.add_argument("--step", choices=("old", "new", "new_sam"))
    ap.add_argument("--dir")
    args = ap.parse_args()
    if args.step:
        out = step_old(args.dir) if args.step == "old" else step_new(args.dir, args.step == "new_sam")
        print(json.dumps(out))
        return
    with tempfile.TemporaryDirectory() as d:
        t0 = time.time()
        synthesize(d, args.parts, args.part_bases, args.reads)
        res = dict(what="predict mode: genome mapping to cluster table", parts=args.parts, part_bases=args.part_bases, reads=args.reads,
                   synthesis_and_index_build_s=round(time.time() - t0, 1))
        sys.stderr.write("world ready after %.0f s\n" % (time.time() - t0))
        res["a_list_text_sort_python"] = child("old", d, args.step_timeout)
        sys.stderr.write("route (a) done\n")
        res["b_cluster_valid_no_sam"] = child("new", d, args.step_timeout)
        res["b_cluster_valid_with_sam"] = child("new_sam", d, args.step_timeout)
    a = res["a_list_text_sort_python"]
    b = res["b_cluster_valid_no_sam"]["second"]
    res["ratio_b_no_sam_over_a_listing_plus_text"] = round(b["total_s"] / (a["second"]["list_valid_s"] + a["second"]["sam_text_s"]), 3)
    res["ratio_b_no_sam_over_a_total"] = round(b["total_s"] / a["total_s"], 4)
    res["command"] = "python scripts/predict_cluster_timing.py --parts %d --part-bases %d --reads %d" % (
        args.parts, args.part_bases, args.reads)
    text = json.dumps(res)
    with open(args.json, "w") as fh:
        fh.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
