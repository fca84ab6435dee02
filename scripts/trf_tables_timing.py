#!/usr/bin/env python3
"""Timing of `annotate -trf`'s typing, selection, cluster assignment and table writing on --reads distinct tRNA reads
(seeded synthetic: --trnas mature tRNAs of 76 nt with predefined tRFs at both ends, one in twenty a duplicate of another,
and as many pre-tRNA trailers of 40 nt; nine reads in ten are pieces of a mature tRNA, a third of them with one `-v 1`
substitution, the others a trailer's first bases followed by 3-12 T's), --samples samples, --runs runs of each route,
alternating, after one warm-up of the array route:

  (a) the record route (the command line's `--trf-host`): columnar.read_subset, trf.collect_trf_content with
      trf.engine_lister (its listing -- pack, upload, Engine.list_best, tuples -- timed apart from the typing),
      trf.write_trf_tables;
  (b) the array route: trf.entry_tables, Engine.trf_classify (count call, filling call, download) on the device-resident
      arrays a cascade leaves behind, columnar.write_trf_tables (row order, mrg_write_trf_tables), trf.content_from_rows.

Host clocks around each stage; `type_kernel_ms` / `assign_kernel_ms` are the two kernels alone between device events inside
mrg_trf_classify, `classify_call_ms` the whole filling call.  The four files of the two routes are compared byte for byte,
and so is the trfContentDic each leaves.  Writes one JSON object to --json (default profiles/trf_tables_timing.json) and
prints it; `passed` = equal files and the slowest run of (b) faster than the fastest run of (a).  Needs a GPU."""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

FILES = ("tRFs.potential.report.tsv", "discarded.reads.summary.assigningtRFs.csv", "tRF.Counts.csv", "tRF.RP100K.csv")


def synthesize(n_trnas, n_reads, n_samples, seed=733):
    from mirge_amd import pack, trf
    rng = np.random.default_rng(seed)
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    T, P = 76, 40
    mat = rng.integers(0, 4, (n_trnas, T), dtype=np.uint8)
    pre = rng.integers(0, 3, (n_trnas, P), dtype=np.uint8)          # (no T inside a trailer: the tail is the read's own)
    dup_of = np.arange(n_trnas)
    for e in range(19, n_trnas, 20):
        dup_of[e] = e - 1
        mat[e], pre[e] = mat[e - 1], pre[e - 1]
    m_names = ["syn-tRNA-%d" % (e + 1) for e in range(n_trnas)]
    p_names = ["pre_syn-tRNA-%d_trailer" % (e + 1) for e in range(n_trnas)]
    m_seqs = [letters[r].tobytes().decode() for r in mat]
    p_seqs = [letters[r].tobytes().decode() for r in pre]
    stru = {n: {"seq": s, "stru": "." * 33 + "XXX" + "." * 40, "anticodonStart": 34, "anticodonEnd": 36} for n, s in zip(m_names, m_seqs)}
    aa = {n: {"aaType": "Gly" if e % 7 else "Und", "anticodon": "GCC"} for e, n in enumerate(m_names)}
    aa.update({n: {"aaType": "Gly" if e % 7 else "Und", "anticodon": "GCC"} for e, n in enumerate(p_names)})
    dup, clusters, merged_name, merged_list = {}, {}, {}, []
    for e in range(n_trnas):
        if dup_of[e] != e:
            dup[m_names[e]], dup[p_names[e]] = m_names[dup_of[e]], p_names[dup_of[e]]
            continue
        if e % 11 == 0:
            continue                                                 # (a tRNA without predefined tRFs: "Dele")
        s = m_seqs[e]
        clusters[m_names[e]] = {trf.add_dash_new(s[:30], T, 1, 30): m_names[e] + "_Cluster1",
                                trf.add_dash_new(s[52:], T, 53, 76): m_names[e] + "_Cluster2"}
        clusters[p_names[e]] = {trf.add_dash_new(p_seqs[e][:20], P, 1, 20): p_names[e] + "_Cluster1"}
        for c, m in ((m_names[e] + "_Cluster1", "_5p"), (m_names[e] + "_Cluster2", "_3p"), (p_names[e] + "_Cluster1", "_trailer")):
            merged_name[c] = m_names[e] + m
            merged_list.append(m_names[e] + m)
    tables = {"trnaStruDic": stru, "trnaAAanticodonDic": aa, "duptRNA2UniqueDic": dup, "tRNAtrfDic": clusters,
              "trfMergedNameDic": merged_name, "trfMergedList": merged_list}
    # reads, oversampled and made distinct
    m = int(n_reads * 1.3) + 1000
    e = rng.integers(0, n_trnas, m)
    trailer = rng.random(m) < 0.1
    L = np.where(trailer, rng.integers(11, 29, m), rng.integers(16, 41, m))
    ends = rng.random(m)
    at = np.where(trailer, 0, np.where(ends < 0.2, 0, np.where(ends < 0.4, T - L, rng.integers(0, T - L + 1))))
    tail = np.where(trailer, rng.integers(3, 13, m), 0)
    width = int((L + tail).max())
    col = np.arange(width)[None, :]
    codes = np.where(trailer[:, None], pre[e[:, None], np.minimum(at[:, None] + col, P - 1)],
                     mat[e[:, None], np.minimum(at[:, None] + col, T - 1)]).astype(np.uint8)
    sub = (~trailer) & (rng.random(m) < 0.33)
    where = rng.integers(0, L)
    codes[sub, where[sub]] = (codes[sub, where[sub]] + rng.integers(1, 4, int(sub.sum()))) & 3
    codes[(col >= L[:, None]) & (col < (L + tail)[:, None])] = 3
    codes[col >= (L + tail)[:, None]] = 7
    _, first = np.unique(codes, axis=0, return_index=True)   # (the padding of 7s carries the length)
    keep = np.sort(first)[:n_reads]
    if keep.size < n_reads:
        raise SystemExit("only %d distinct reads: raise --trnas" % keep.size)
    codes, trailer, full = codes[keep], trailer[keep], (L + tail)[keep]
    words = np.zeros((2, n_reads), dtype=np.uint64)
    for L_ in np.unique(full):
        rows = np.nonzero(full == L_)[0]
        words[:, rows] = pack.pack_codes(codes[rows, :int(L_)], 2)[0]
    quant = rng.integers(0, 6, (n_reads, n_samples)).astype(np.uint32)
    quant[quant.sum(axis=1) == 0, 0] = 1
    reads_per_sample = quant.sum(axis=0)
    return dict(libs={"mature_trna": (m_names, m_seqs), "pre_trna": (p_names, p_seqs)}, tables=tables, pre=dict(zip(p_names, p_seqs)),
                words=words, lens=full.astype(np.uint8), pass_id=np.where(trailer, 3, 2).astype(np.int8),
                ref_id=np.zeros(n_reads, dtype=np.int32), pos=np.zeros(n_reads, dtype=np.int32), mm=np.zeros(n_reads, dtype=np.uint8),
                quant=quant, log_dic={"quantStats": [{"maturetrnaReads": int(x), "pretrnaReads": 0} for x in reads_per_sample]})


def record_route(w, eng, outdir, sample_list):
    from mirge_amd import columnar, trf
    t0 = time.time()
    npp = [None, None, w["libs"]["mature_trna"][0], w["libs"]["pre_trna"][0]]
    sub, _ = columnar.read_subset(w["words"], w["lens"], None, w["quant"], w["pass_id"], w["ref_id"], w["pos"], w["mm"], npp, {2, 3})
    t1 = time.time()
    inner = trf.engine_lister(eng)
    spent = [0.0]

    def lister(reads, key, v):
        a = time.time()
        out = inner(reads, key, v)
        spent[0] += time.time() - a
        return out
    content = {}
    trf.collect_trf_content(content, sub, sample_list, w["tables"]["trnaStruDic"], w["pre"], lister)
    t2 = time.time()
    trf.write_trf_tables(outdir, sample_list, w["log_dic"], content, w["tables"], w["pre"])
    t3 = time.time()
    return dict(read_subset_s=t1 - t0, engine_lister_s=spent[0], typing_s=t2 - t1 - spent[0], write_trf_tables_s=t3 - t2,
                total_s=t3 - t0), content


def array_route(w, dev, eng, outdir, sample_list):
    import torch
    from mirge_amd import columnar, pack, trf
    torch.cuda.synchronize()
    t0 = time.time()
    et = trf.entry_tables(w["libs"]["mature_trna"][0], w["libs"]["pre_trna"][0], w["tables"], w["pre"])
    t1 = time.time()
    timings = {}
    rec, hits, n2, n3 = eng.trf_classify(et, dev["words"], dev["lens"], None, dev["pass_id"], timings=timings)
    t2 = time.time()
    t_rec, lines = columnar.write_trf_tables(outdir, sample_list, w["log_dic"], w["words"], w["lens"], None, w["quant"], rec, hits, n2, et)
    t3 = time.time()
    idx = t_rec[:, 0]
    seqs = pack.unpack_reads(np.ascontiguousarray(w["words"][:, idx]), w["lens"][idx], None)
    denom = [q["maturetrnaReads"] + q["pretrnaReads"] for q in w["log_dic"]["quantStats"]]
    content = trf.content_from_rows(et, t_rec, seqs, w["quant"][idx], denom)
    t4 = time.time()
    return dict(entry_tables_s=t1 - t0, classify_and_download_s=t2 - t1, classify_call_ms=timings.get("classify_call_ms"),
                type_kernel_ms=timings.get("type_kernel_ms"), assign_kernel_ms=timings.get("assign_kernel_ms"),
                order_and_write_s=t3 - t2, content_from_rows_s=t4 - t3, total_s=t4 - t0, rows=int(n2 + n3), kept_alignments=int(hits.shape[0]),
                lines=lines), content


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1000000)
    ap.add_argument("--trnas", type=int, default=4000)
    ap.add_argument("--samples", type=int, default=2)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "trf_tables_timing.json"))
    args = ap.parse_args()
    import torch
    from mirge_amd.engine import Engine
    from mirge_amd.index import FmIndex
    eng = Engine(0)          # (raises without a GPU)
    t0 = time.time()
    w = synthesize(args.trnas, args.reads, args.samples)
    for key in ("mature_trna", "pre_trna"):
        eng.add_library(key, FmIndex.build(*w["libs"][key]))
    print("synthesised %d reads on %d tRNAs in %.1f s" % (args.reads, args.trnas, time.time() - t0), flush=True)
    dev = {k: torch.from_numpy(w[k].view(np.int64) if k == "words" else w[k]).to(eng.device) for k in ("words", "lens", "pass_id")}
    sample_list = ["s%d.fastq" % i for i in range(args.samples)]
    out = dict(what="annotate -trf: typing, selection, cluster assignment and the four tRF tables", reads=args.reads, trnas=args.trnas,
               samples=args.samples, record_route=[], array_route=[], command="python scripts/trf_tables_timing.py " + " ".join(sys.argv[1:]))
    with tempfile.TemporaryDirectory() as d:
        a_dir, b_dir = os.path.join(d, "a"), os.path.join(d, "b")
        os.mkdir(a_dir)
        os.mkdir(b_dir)
        array_route(w, dev, eng, b_dir, sample_list)    # warm-up: code objects
        for run in range(args.runs):
            r, old_content = record_route(w, eng, a_dir, sample_list)
            out["record_route"].append(r)
            print("run %d record route %.2f s" % (run, r["total_s"]), flush=True)
            r, new_content = array_route(w, dev, eng, b_dir, sample_list)
            out["array_route"].append(r)
            print("run %d array route %.3f s" % (run, r["total_s"]), flush=True)
        same = True
        for fn in FILES:
            same &= open(os.path.join(a_dir, fn), "rb").read() == open(os.path.join(b_dir, fn), "rb").read()
            out.setdefault("file_bytes", []).append(os.path.getsize(os.path.join(b_dir, fn)))
        out["content_equal"] = bool(old_content == new_content and list(old_content) == list(new_content))
    old = [r["total_s"] for r in out["record_route"]]
    new = [r["total_s"] for r in out["array_route"]]
    out["files_equal"] = bool(same)
    out["record_fastest_s"], out["array_slowest_s"] = min(old), max(new)
    out["ratio_record_fastest_over_array_slowest"] = round(min(old) / max(new), 1)
    out["passed"] = bool(same and out["content_equal"] and max(new) < min(old))
    text = json.dumps(out)
    with open(args.json, "w") as fh:
        fh.write(text + "\n")
    print(text)
    return 0 if out["passed"] else 1


if __name__ == "__main__":
    sys.exit(main())
