#!/usr/bin/env python3
"""Timing of `annotate --novel-clusters` after the tables are written: from unmapped.csv / the arrays to the candidate
FASTA files and every sample's location clusters.  Input (seeded synthetic): --reads distinct unmapped reads of 16-40 nt cut
in piles from either strand of a random genome of --chroms x --chrom-bases bases (one read in 200 with an N), zipf counts
over --samples samples with a third of the cells empty.  --runs runs of each route, alternating, after one warm-up of the
array route:

  (a) the host route: the plain-Python model (tests/predict_reads_model.py) over the text of the written unmapped.csv --
      it stands in for the reference's convert2Fasta, which reads the same file the same way, one line at a time -- then
      predict.map_and_cluster from each sample's FASTA file;
  (b) the array route: predict.candidate_lists on the device-resident arrays (mrg_predict_select once,
      mrg_predict_sample_reads per sample and list, the lists downloaded), predict.write_candidate_reads
      (mrg_write_predict_fasta), then per sample Engine.predict_gather and predict.map_and_cluster_reads.

Host clocks around each route and its stages; `select_ms` / `samples_ms` / `gather_ms` between device events.  Every file of
the two routes is compared byte for byte.  Writes one JSON object to --json (default profiles/novel_reads_timing.json) and
prints it; `passed` = equal files.  Needs a GPU."""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

ANNOT_NAMES = ["exact miRNA", "hairpin miRNA", "mature tRNA", "primary tRNA", "snoRNA", "rRNA", "ncrna others", "mRNA",
               "isomiR miRNA"]


def synthesize(n_reads, n_samples, n_chroms, chrom_bases, seed=1502):
    from mirge_amd import pack
    rng = np.random.default_rng(seed)
    genome = rng.integers(0, 4, (n_chroms, chrom_bases), dtype=np.uint8)
    m = int(n_reads * 1.05) + 1000
    loci = rng.integers(100, chrom_bases - 100, max(1000, n_reads // 6))
    pick = rng.integers(0, loci.size, m)
    pos = loci[pick] + rng.integers(-30, 31, m)
    chrom = rng.integers(0, n_chroms, loci.size)[pick]
    L = rng.integers(16, 41, m)
    minus = rng.random(m) < 0.5
    with_n = rng.random(m) < 0.005
    words = np.zeros((2, m), dtype=np.uint64)
    nmask = np.zeros((2, m), dtype=np.uint64)
    for L_ in np.unique(L):
        rows = np.nonzero(L == L_)[0]
        sub = genome[chrom[rows, None], pos[rows, None] + np.arange(int(L_))[None, :]]
        rc = minus[rows]
        sub[rc] = 3 - sub[rc][:, ::-1]
        hit = np.nonzero(with_n[rows])[0]
        sub[hit, rng.integers(0, int(L_), hit.size)] = 4
        w, _, nm = pack.pack_codes(sub, 2)
        words[:, rows] = w
        if nm is not None:
            nmask[:, rows] = nm
    key = np.stack([words[0], words[1], nmask[0], nmask[1], L.astype(np.uint64)], axis=1)
    _, first = np.unique(key, axis=0, return_index=True)
    keep = np.sort(first)[:n_reads]
    if keep.size < n_reads:
        raise SystemExit("only %d distinct reads" % keep.size)
    quant = np.minimum(rng.zipf(1.5, size=(n_reads, n_samples)), 2 ** 32 - 1).astype(np.uint32)
    quant[rng.random(quant.shape) < 0.33] = 0
    names = ["chr%d" % (i + 1) for i in range(n_chroms)]
    texts = [np.frombuffer(b"ACGT", dtype=np.uint8)[g].tobytes().decode() for g in genome]
    return dict(words=np.ascontiguousarray(words[:, keep]), lens=L[keep].astype(np.uint8),
                nmask=np.ascontiguousarray(nmask[:, keep]), quant=quant, pass_id=np.full(n_reads, -1, np.int8)), names, texts


def host_route(eng, csv_path, outdir, genome, policy):
    from mirge_amd import predict
    from tests import predict_reads_model as model
    t0 = time.time()
    with open(csv_path) as fh:
        samples, seqs, quant = model.from_csv(fh.read())
    files = model.files(samples, seqs, quant, *policy[:3])
    for fn, text in files.items():
        with open(os.path.join(outdir, fn), "w") as fh:
            fh.write(text)
    t1 = time.time()
    for name in samples:
        stem = "unmapped_mirna_" + model.stem(name)
        predict.map_and_cluster(eng, os.path.join(outdir, stem + ".fa"), genome, *policy[3:], os.path.join(outdir, stem))
    t2 = time.time()
    return dict(model_over_csv_s=t1 - t0, map_and_cluster_s=t2 - t1, total_s=t2 - t0)


def array_route(eng, w, dev, outdir, sample_list, genome, policy):
    import torch
    from mirge_amd import predict
    torch.cuda.synchronize()
    t0 = time.time()
    timings = {}
    lists = predict.candidate_lists(eng, dev["pass_id"], dev["lens"], dev["quant"], *policy[:3], timings=timings)
    t1 = time.time()
    rows = predict.write_candidate_reads(outdir, sample_list, w["words"], w["lens"], w["nmask"], lists, *policy[:3])
    t2 = time.time()
    gather_ms = 0.0
    for s, name in enumerate(sample_list):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g = eng.predict_gather(dev["words"], dev["lens"], dev["nmask"], dev["quant"], lists["sample_sel"][s][0], sample=s)
        e1.record()
        e1.synchronize()
        gather_ms += e0.elapsed_time(e1)
        predict.map_and_cluster_reads(eng, g[:3], lists["sample_sel"][s][1], g[3], genome, *policy[3:],
                                      os.path.join(outdir, "unmapped_mirna_" + predict.sample_stem(name)))
    t3 = time.time()
    return dict(lists_and_download_s=t1 - t0, select_ms=timings["select_ms"], samples_ms=timings["samples_ms"], writer_s=t2 - t1,
                gather_ms=gather_ms, map_and_cluster_s=t3 - t2, total_s=t3 - t0, rows=rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=2000000)
    ap.add_argument("--samples", type=int, default=2)
    ap.add_argument("--chroms", type=int, default=4)
    ap.add_argument("--chrom-bases", type=int, default=2000000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "novel_reads_timing.json"))
    args = ap.parse_args()
    import torch
    from mirge_amd import columnar
    from mirge_amd.engine import Engine
    from mirge_amd.index import FmIndex
    eng = Engine(0)          # (raises without a GPU)
    t0 = time.time()
    w, names, texts = synthesize(args.reads, args.samples, args.chroms, args.chrom_bases)
    print("synthesised %d reads in %.1f s" % (args.reads, time.time() - t0), flush=True)
    dev = {k: torch.from_numpy(w[k].view({"quant": np.int32, "words": np.int64, "nmask": np.int64}.get(k, w[k].dtype))).to(eng.device)
           for k in ("words", "lens", "nmask", "quant", "pass_id")}
    sample_list = ["s%d.fastq" % i for i in range(args.samples)]
    policy = (16, 25, 2, 3, 25, 14)     # -minl -maxl -cc -ml -sl -olc
    out = dict(what="annotate --novel-clusters: candidate reads and location clusters from unmapped.csv / from the arrays",
               reads=args.reads, samples=args.samples, genome_bases=args.chroms * args.chrom_bases, host_route=[], array_route=[],
               command="python scripts/novel_reads_timing.py " + " ".join(sys.argv[1:]))
    with tempfile.TemporaryDirectory() as d:
        genome = os.path.join(d, "syn_genome")
        t0 = time.time()
        FmIndex.build(names, texts).save(genome + ".mrgfm")
        print("genome index in %.1f s" % (time.time() - t0), flush=True)
        t0 = time.time()
        columnar.write_read_tables(d, ANNOT_NAMES, sample_list, w["words"], w["lens"], w["nmask"], w["quant"], w["pass_id"],
                                   np.full(args.reads, -1, np.int32), [[] for _ in ANNOT_NAMES])
        csv_path = os.path.join(d, "unmapped.csv")
        out["unmapped_csv_bytes"] = os.path.getsize(csv_path)
        print("unmapped.csv (%d bytes) in %.1f s" % (out["unmapped_csv_bytes"], time.time() - t0), flush=True)
        a_dir, b_dir = os.path.join(d, "a"), os.path.join(d, "b")
        os.mkdir(a_dir)
        os.mkdir(b_dir)
        array_route(eng, w, dev, b_dir, sample_list, genome, policy)    # warm-up: code objects, the genome's upload
        for run in range(args.runs):
            r = host_route(eng, csv_path, a_dir, genome, policy)
            out["host_route"].append(r)
            print("run %d host route %.2f s" % (run, r["total_s"]), flush=True)
            r = array_route(eng, w, dev, b_dir, sample_list, genome, policy)
            out["array_route"].append(r)
            print("run %d array route %.3f s" % (run, r["total_s"]), flush=True)
        same, sizes = True, {}
        assert sorted(os.listdir(a_dir)) == sorted(os.listdir(b_dir)) and len(os.listdir(a_dir)) == 2 + 4 * args.samples
        for fn in sorted(os.listdir(a_dir)):
            with open(os.path.join(a_dir, fn), "rb") as f1, open(os.path.join(b_dir, fn), "rb") as f2:
                same &= f1.read() == f2.read()
            sizes[fn] = os.path.getsize(os.path.join(b_dir, fn))
        out["file_bytes"] = sizes
    old = [r["total_s"] for r in out["host_route"]]
    new = [r["total_s"] for r in out["array_route"]]
    out["files_equal"] = bool(same)
    out["host_fastest_s"], out["array_slowest_s"] = min(old), max(new)
    out["ratio_host_fastest_over_array_slowest"] = round(min(old) / max(new), 1)
    out["passed"] = bool(same)
    text = json.dumps(out)
    with open(args.json, "w") as fh:
        fh.write(text + "\n")
    print(text)
    return 0 if out["passed"] else 1


if __name__ == "__main__":
    sys.exit(main())
