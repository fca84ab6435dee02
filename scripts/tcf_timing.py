#!/usr/bin/env python3
"""Timing of `annotate -tcf` (<sample>.trim.collapse.fa) on --reads distinct reads of 16-40 nt (seeded synthetic: one base
in fifty an N, zipf counts over --samples samples, a third of the cells empty), --runs runs of each route, alternating,
after one warm-up of the array route:

  (a) the host route (the command line's `--tcf-host`): report.write_collapsed_fa_host -- pack.unpack_reads over the
      sample's reads, sorted((count, sequence)) reversed, a formatted write per row;
  (b) the array route: Engine.collapsed_order on the device-resident arrays a collapse leaves behind (mrg_seq_rank once,
      mrg_collapsed_order per sample, the orders downloaded), columnar.write_collapsed_fa (mrg_write_collapsed_fasta).

Host clocks around each route and, for (b), around its two stages; `rank_ms` / `order_ms` are the string rank and the
per-sample orders between device events.  The files of the two routes are compared byte for byte.  Writes one JSON object
to --json (default profiles/tcf_timing.json) and prints it; `passed` = equal files and the slowest run of (b) not slower
than the fastest run of (a).  Needs a GPU."""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def synthesize(n_reads, n_samples, seed=447):
    from mirge_amd import pack
    rng = np.random.default_rng(seed)
    m = int(n_reads * 1.02) + 1000
    L = rng.integers(16, 41, m)
    codes = rng.integers(0, 4, (m, 40), dtype=np.uint8)
    codes[rng.random((m, 40)) < 0.02] = 4                      # N
    codes[np.arange(40)[None, :] >= L[:, None]] = 7            # (the padding carries the length)
    _, first = np.unique(codes, axis=0, return_index=True)
    keep = np.sort(first)[:n_reads]
    if keep.size < n_reads:
        raise SystemExit("only %d distinct reads" % keep.size)
    codes, L = codes[keep], L[keep]
    words = np.zeros((2, n_reads), dtype=np.uint64)
    nmask = np.zeros((2, n_reads), dtype=np.uint64)
    for L_ in np.unique(L):
        rows = np.nonzero(L == L_)[0]
        w, _, nm = pack.pack_codes(codes[rows, :int(L_)], 2)
        words[:, rows] = w
        if nm is not None:
            nmask[:, rows] = nm
    quant = np.minimum(rng.zipf(1.5, size=(n_reads, n_samples)), 2 ** 32 - 1).astype(np.uint32)
    quant[rng.random(quant.shape) < 0.33] = 0
    quant[quant.sum(axis=1) == 0, 0] = 1
    return dict(words=words, lens=L.astype(np.uint8), nmask=nmask, quant=quant)


def host_route(w, outdir, sample_list):
    from mirge_amd import report
    t0 = time.time()
    report.write_collapsed_fa_host(outdir, sample_list, w["words"], w["lens"], w["nmask"], w["quant"], {})
    return dict(total_s=time.time() - t0)


def array_route(w, dev, eng, outdir, sample_list):
    import torch
    from mirge_amd import columnar
    torch.cuda.synchronize()
    t0 = time.time()
    timings = {}
    orders = eng.collapsed_order(dev["words"], dev["lens"], dev["nmask"], dev["quant"], timings=timings)
    t1 = time.time()
    rows = columnar.write_collapsed_fa(outdir, sample_list, w["words"], w["lens"], w["nmask"], w["quant"], orders, {})
    t2 = time.time()
    return dict(order_and_download_s=t1 - t0, rank_ms=timings["rank_ms"], order_ms=timings["order_ms"], writer_s=t2 - t1,
                total_s=t2 - t0, rows=rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=2000000)
    ap.add_argument("--samples", type=int, default=2)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "tcf_timing.json"))
    args = ap.parse_args()
    import torch
    from mirge_amd.engine import Engine
    eng = Engine(0)          # (raises without a GPU)
    t0 = time.time()
    w = synthesize(args.reads, args.samples)
    print("synthesised %d reads in %.1f s" % (args.reads, time.time() - t0), flush=True)
    dev = {k: torch.from_numpy(w[k].view(np.int32 if k == "quant" else np.int64) if k != "lens" else w[k]).to(eng.device)
           for k in ("words", "lens", "nmask", "quant")}
    sample_list = ["s%d.fastq" % i for i in range(args.samples)]
    out = dict(what="annotate -tcf: the order of the collapsed reads and <sample>.trim.collapse.fa", reads=args.reads,
               samples=args.samples, host_route=[], array_route=[], command="python scripts/tcf_timing.py " + " ".join(sys.argv[1:]))
    with tempfile.TemporaryDirectory() as d:
        a_dir, b_dir = os.path.join(d, "a"), os.path.join(d, "b")
        os.mkdir(a_dir)
        os.mkdir(b_dir)
        array_route(w, dev, eng, b_dir, sample_list)    # warm-up: code objects
        for run in range(args.runs):
            r = host_route(w, a_dir, sample_list)
            out["host_route"].append(r)
            print("run %d host route %.2f s" % (run, r["total_s"]), flush=True)
            r = array_route(w, dev, eng, b_dir, sample_list)
            out["array_route"].append(r)
            print("run %d array route %.3f s" % (run, r["total_s"]), flush=True)
        same = True
        for s in sample_list:
            fn = os.path.splitext(s)[0] + ".trim.collapse.fa"
            with open(os.path.join(a_dir, fn), "rb") as f1, open(os.path.join(b_dir, fn), "rb") as f2:
                same &= f1.read() == f2.read()
            out.setdefault("file_bytes", []).append(os.path.getsize(os.path.join(b_dir, fn)))
    old = [r["total_s"] for r in out["host_route"]]
    new = [r["total_s"] for r in out["array_route"]]
    out["files_equal"] = bool(same)
    out["host_fastest_s"], out["array_slowest_s"] = min(old), max(new)
    out["ratio_host_fastest_over_array_slowest"] = round(min(old) / max(new), 1)
    out["passed"] = bool(same and max(new) <= min(old))
    text = json.dumps(out)
    with open(args.json, "w") as fh:
        fh.write(text + "\n")
    print(text)
    return 0 if out["passed"] else 1


if __name__ == "__main__":
    sys.exit(main())
