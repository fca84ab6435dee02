#!/usr/bin/env python3
"""Timing of `annotate -gff`'s classification and writing on --reads distinct reads on miRNA entries (seeded synthetic:
--entries entries cut from their own hairpins; every read is an entry's mature sequence with end shifts of -3 .. +3 on
either side and 0-2 substitutions, claimed by the exact-miRNA or the isomiR pass at the offset an aligner would report),
--samples samples, --runs runs of each route, alternating:

  (a) the record route (the command line's `--gff-host`): columnar.read_subset, isomir.build_isomir_content for the two
      passes, isomir.write_isomir_gff;
  (b) the array route: isomir.entry_table, Engine.isomir_classify (count call, fill call, download of the rows) on the
      device-resident arrays a cascade leaves behind, columnar.write_isomir_gff (mrg_write_isomir_gff).

Host clocks around each route (route (b) ends in the download, which synchronises); `kernel_ms` is
classify_kernel alone between two device events inside mrg_isomir_classify, `classify_call_ms` the whole filling call.  The files of the two routes are compared byte for byte.  Writes one
JSON object to --json (default profiles/isomir_gff_timing.json) and prints it; `passed` = the slowest run of (b) is faster
than the fastest run of (a).  Needs a GPU: there is no fallback."""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def synthesize(n_entries, n_reads, n_samples, seed=621):
    rng = np.random.default_rng(seed)
    HP, M0, ML = 80, 15, 22
    hp = rng.integers(0, 4, (n_entries, HP), dtype=np.uint8)
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    hp_txt = [letters[row].tobytes().decode() for row in hp]
    names = ["syn-miR-%d-5p" % (e + 1) for e in range(n_entries)]
    seqs = [t[M0 - 2:M0 + ML + 6] for t in hp_txt]
    hairpin = {"syn-mir-%d" % (e + 1): t for e, t in enumerate(hp_txt)}
    # reads, oversampled and made distinct
    m = int(n_reads * 1.5) + 1000
    e = rng.integers(0, n_entries, m)
    d5, d3 = rng.integers(-3, 4, m), rng.integers(-3, 4, m)
    r0, L = M0 + d5, ML - d5 + d3
    width = int(L.max())
    col = np.arange(width)[None, :]
    codes = hp[e[:, None], np.minimum(r0[:, None] + col, HP - 1)]
    n_sub = rng.integers(0, 3, m)
    for k in range(2):
        at = rng.integers(0, L)
        hit = n_sub > k
        codes[hit, at[hit]] = (codes[hit, at[hit]] + rng.integers(1, 4, int(hit.sum()))) & 3
    codes[col >= L[:, None]] = 7
    _, first = np.unique(codes, axis=0, return_index=True)   # (the padding of 7s carries the length)
    keep = np.sort(first)[:n_reads]
    if keep.size < n_reads:
        raise SystemExit("only %d distinct reads: raise --entries" % keep.size)
    e, d5, L, codes = e[keep], d5[keep], L[keep], codes[keep]
    iso = (d5 < -2) | (rng.random(n_reads) < 0.5)
    pass_id = np.where(iso, 8, 0).astype(np.int8)
    pos = (2 + d5 + iso).astype(np.int32)
    from mirge_amd import pack
    words = np.zeros((1, n_reads), dtype=np.uint64)
    for L_ in np.unique(L):
        rows = np.nonzero(L == L_)[0]
        words[:, rows] = pack.pack_codes(codes[rows, :int(L_)], 1)[0]
    quant = rng.integers(0, 6, (n_reads, n_samples)).astype(np.uint32)
    quant[quant.sum(axis=1) == 0, 0] = 1
    return dict(names=names, seqs=seqs, hairpin=hairpin, words=words, lens=L.astype(np.uint8), pass_id=pass_id,
                ref_id=e.astype(np.int32), pos=pos, mm=np.zeros(n_reads, dtype=np.uint8), quant=quant)


def record_route(w, outdir, sample_list):
    from mirge_amd import columnar, isomir
    t0 = time.time()
    npp = [w["names"]] * 9
    sub, align = columnar.read_subset(w["words"], w["lens"], None, w["quant"], w["pass_id"], w["ref_id"], w["pos"], w["mm"], npp,
                                      {0, 8})
    t1 = time.time()
    content = {}
    mirna_seqs = dict(zip(w["names"], w["seqs"]))
    for pass_index in (0, 8):
        trim = 0 if pass_index == 0 else 3
        hits = {s: (npp[pass_index][a[1]], a[2] + 1, "%dM" % (len(s) - trim)) for s, a in align.items() if a[0] == pass_index}
        isomir.build_isomir_content(content, hits, pass_index, {}, w["hairpin"], mirna_seqs, "miRBase")
    t2 = time.time()
    isomir.write_isomir_gff(outdir, sample_list, content, sub, "miRBase")
    t3 = time.time()
    return dict(read_subset_s=t1 - t0, build_isomir_content_s=t2 - t1, write_isomir_gff_s=t3 - t2, total_s=t3 - t0)


def array_route(w, dev, eng, outdir, sample_list):
    import torch
    from mirge_amd import columnar, isomir
    torch.cuda.synchronize()
    t0 = time.time()
    table = isomir.entry_table(w["names"], w["seqs"], w["hairpin"], {}, "miRBase")
    t1 = time.time()
    timings = {}
    idx, rec, mask, n_canon, n_iso = eng.isomir_classify(table, dev["words"], dev["lens"], None, dev["pass_id"], dev["ref_id"],
                                                         dev["pos"], timings=timings)
    t2 = time.time()
    lines = columnar.write_isomir_gff(outdir, sample_list, w["words"], w["lens"], None, w["quant"], idx, rec, mask, table, w["names"],
                                      "miRBase")
    t3 = time.time()
    return dict(entry_table_s=t1 - t0, classify_and_download_s=t2 - t1, kernel_ms=timings.get("kernel_ms"), classify_call_ms=timings.get("classify_call_ms"), write_s=t3 - t2,
                total_s=t3 - t0, rows=int(n_canon + n_iso), lines=lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1000000)
    ap.add_argument("--entries", type=int, default=20000)
    ap.add_argument("--samples", type=int, default=2)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "isomir_gff_timing.json"))
    args = ap.parse_args()
    import torch
    from mirge_amd.engine import Engine
    eng = Engine(0)          # (raises without a GPU)
    t0 = time.time()
    w = synthesize(args.entries, args.reads, args.samples)
    print("synthesised %d reads on %d entries in %.1f s" % (args.reads, args.entries, time.time() - t0), flush=True)
    dev = {k: torch.from_numpy(w[k].view(np.int64) if k == "words" else w[k]).to(eng.device)
           for k in ("words", "lens", "pass_id", "ref_id", "pos")}
    sample_list = ["s%d.fastq" % i for i in range(args.samples)]
    out = dict(what="annotate -gff: classification and GFF files", reads=args.reads, entries=args.entries, samples=args.samples,
               record_route=[], array_route=[], command="python scripts/isomir_gff_timing.py " + " ".join(sys.argv[1:]))
    with tempfile.TemporaryDirectory() as d:
        a_dir, b_dir = os.path.join(d, "a"), os.path.join(d, "b")
        os.mkdir(a_dir)
        os.mkdir(b_dir)
        array_route(w, dev, eng, b_dir, sample_list)    # warm-up: code objects, the context's scratch
        for run in range(args.runs):
            out["record_route"].append(record_route(w, a_dir, sample_list))
            print("run %d record route %.2f s" % (run, out["record_route"][-1]["total_s"]), flush=True)
            out["array_route"].append(array_route(w, dev, eng, b_dir, sample_list))
            print("run %d array route %.3f s" % (run, out["array_route"][-1]["total_s"]), flush=True)
        same = True
        for s in sample_list:
            fn = os.path.splitext(s)[0] + "_isomiRs.gff"
            same &= open(os.path.join(a_dir, fn), "rb").read() == open(os.path.join(b_dir, fn), "rb").read()
            out.setdefault("file_bytes", []).append(os.path.getsize(os.path.join(b_dir, fn)))
    old = [r["total_s"] for r in out["record_route"]]
    new = [r["total_s"] for r in out["array_route"]]
    out["files_equal"] = bool(same)
    out["record_fastest_s"], out["array_slowest_s"] = min(old), max(new)
    out["ratio_record_fastest_over_array_slowest"] = round(min(old) / max(new), 1)
    out["passed"] = bool(same and max(new) < min(old))
    text = json.dumps(out)
    with open(args.json, "w") as fh:
        fh.write(text + "\n")
    print(text)
    return 0 if out["passed"] else 1


if __name__ == "__main__":
    sys.exit(main())
