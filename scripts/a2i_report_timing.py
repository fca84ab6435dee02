#!/usr/bin/env python3
"""Timing of `annotate -ai`'s report on --reads distinct miRNA reads (seeded synthetic: --mirnas miRNAs of 19-25 nt, one in
ten low-complexity, each inside its own stretch of one synthetic chromosome; a read is its miRNA with a 5' shift of +-2, a
3' shift of +-3, 0-2 substitutions, one read in ten with a deleted base, 0-2 added bases; the miRNA's own sequence is the
exact-pass read, the others belong to the isomiR pass), --samples samples in which every read is present, --runs runs of
each route, alternating, after one warm-up of the array route:

  (a) the record route (the command line's `--ai-host`): columnar.read_subset, a2i.a_to_i_report (one local_pair per
      miRNA, sample and read) with a2i.EngineGenome's string forms;
  (b) the array route: a2i.target_table, a2i.keep_mask, Engine.a2i_align (count call, filling call, download) on the
      device-resident arrays a cascade leaves behind, a2i.a_to_i_report_arrays (numpy over the records, the packed genome
      filter, mrg_write_a2i_detail, a2i_editing on the blocks that hold a read the kernel did not settle).

Host clocks around each stage; `kernel_ms` is the alignment kernel alone between device events inside mrg_a2i_align,
`align_call_ms` the whole filling call, `genome_s` the time inside the genome filters (both routes run them on the GPU),
`host_blocks_s` the time a2i_editing takes on the `host_blocks` of `blocks` (miRNA, sample) blocks that hold a read the
kernel did not settle, `detail_write_s` mrg_write_a2i_detail.
A third leg, --settle-runs runs of each, alternating: route (b) without and with `settle` (mrg_a2i_settle settles the
tied pairs on the device before the download); per run also `settle_examined`, `settle_settled`, `settle_kernel_ms` and
`tied_rows`.  `settle_leg` holds the runs, the median wall times and their ratio.
The three files of all routes are compared byte for byte.  Writes one JSON object to --json (default
profiles/a2i_report_timing.json) and prints it; `passed` = equal files, the slowest run of (b) faster than the fastest
run of (a), and fewer host blocks with `settle` than without.  --record-runs (default --runs) runs route (a) fewer times
than (b).  Needs a GPU."""
import argparse
import json
import os
import random
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

FILES = ("a2IEditing.detail.txt", "a2IEditing.report.csv", "a2IEditing.report.newform.csv")


def synthesize(n_mirnas, n_reads, n_samples, seed=911):
    from mirge_amd import pack
    rnd = random.Random(seed)
    rng = np.random.default_rng(seed)
    names, targets, chrom = [], [], []
    per = -(-n_reads // n_mirnas) + 2
    reads = {}
    for e in range(n_mirnas):
        alpha = rnd.choice(["AC", "AAG", "AT"]) if rnd.random() < 0.1 else "ACGT"
        L = rnd.randint(19, 25)
        pre = "".join(rnd.choice("ACGT") for _ in range(30)) + "".join(rnd.choice(alpha) for _ in range(L)) + \
            "".join(rnd.choice("ACGT") for _ in range(30))
        target = pre[30:30 + L]
        names.append("syn-miR-%d" % (e + 1))
        targets.append(target)
        chrom.append(pre)
        if target not in reads:
            reads[target] = (0, e)
        tries = 0
        made = 0
        while made < per and tries < 20 * per:
            tries += 1
            s = list(pre[30 + rnd.randint(-2, 2):30 + L + rnd.randint(-3, 3)])
            for _ in range(rnd.randint(0, 2)):
                s[rnd.randrange(len(s))] = rnd.choice("ACGT")
            if rnd.random() < 0.1:
                del s[rnd.randrange(3, len(s) - 3)]
            s = "".join(s) + "".join(rnd.choice("ACGT") for _ in range(rnd.randint(0, 2)))
            if s not in reads:
                reads[s] = (8, e)
                made += 1
    seqs = list(reads)[:n_reads]
    if len(seqs) < n_reads:
        raise SystemExit("only %d distinct reads: raise --mirnas" % len(seqs))
    order = rng.permutation(n_reads)
    seqs = [seqs[i] for i in order]
    pass_id = np.array([reads[s][0] for s in seqs], dtype=np.int8)
    ref_id = np.array([reads[s][1] for s in seqs], dtype=np.int32)
    words, lens, nmask = pack.pack_reads(seqs)
    quant = rng.integers(1, 40, (n_reads, n_samples)).astype(np.uint32)
    total = np.zeros((n_mirnas, n_samples), dtype=np.int64)
    np.add.at(total, ref_id, quant)
    mir_dic = {n: {"quant": [int(x) for x in total[e]], "iscan": [int(x) for x in total[e]]} for e, n in enumerate(names)}
    log_dic = {"quantStats": [{"mirnaReadsFiltered": int(x)} for x in quant.sum(axis=0)]}
    return dict(names=names, name_seq=dict(zip(names, targets)), genome=("chrS", "".join(chrom)), words=words, lens=lens, nmask=nmask,
                quant=quant, pass_id=pass_id, ref_id=ref_id, pos=np.zeros(n_reads, np.int32), mm=np.zeros(n_reads, np.uint8),
                mir_dic=mir_dic, log_dic=log_dic, removed=names[3::97])


class TimedGenome:
    """A genome filter that adds up the time spent inside it."""

    def __init__(self, inner):
        self.inner, self.spent = inner, 0.0

    def _timed(self, fn, *a):
        t = time.time()
        out = fn(*a)
        self.spent += time.time() - t
        return out

    def unique_best(self, reads):
        return self._timed(self.inner.unique_best, reads)

    def exact_hit(self, reads):
        return self._timed(self.inner.exact_hit, reads)

    def unique_best_mask(self, *a):
        return self._timed(self.inner.unique_best_mask, *a)


def record_route(w, genome, outdir, sample_list):
    from mirge_amd import a2i, columnar
    g = TimedGenome(genome)
    t0 = time.time()
    npp = [w["names"]] * 9
    sub, _ = columnar.read_subset(w["words"], w["lens"], w["nmask"], w["quant"], w["pass_id"], w["ref_id"], w["pos"], w["mm"], npp, {0, 8})
    t1 = time.time()
    a2i.a_to_i_report(outdir, sample_list, w["log_dic"], sub, w["mir_dic"], w["name_seq"], {}, w["removed"], g)
    t2 = time.time()
    return dict(read_subset_s=t1 - t0, genome_s=g.spent, report_s=t2 - t1 - g.spent, total_s=t2 - t0)


def array_route(w, dev, eng, genome, outdir, sample_list, settle=False):
    import torch
    from mirge_amd import a2i
    g = TimedGenome(genome)
    torch.cuda.synchronize()
    t0 = time.time()
    table = a2i.target_table([w["names"]] * 9, {}, w["name_seq"])
    keep = a2i.keep_mask(w["quant"], w["pass_id"], w["log_dic"])
    t1 = time.time()
    timings = {}
    idx, rec = eng.a2i_align(table, dev["words"], dev["lens"], dev["nmask"], dev["pass_id"], dev["ref_id"], keep, timings=timings,
                             settle=settle)
    t2 = time.time()
    a2i.a_to_i_report_arrays(outdir, sample_list, w["log_dic"], w["words"], w["lens"], w["nmask"], w["quant"], w["pass_id"], idx, rec,
                             table, w["mir_dic"], w["name_seq"], w["removed"], g, timings=timings)
    t3 = time.time()
    status = rec[:, 0] & 0xFF
    out = dict(tables_s=t1 - t0, align_and_download_s=t2 - t1, align_call_ms=timings.get("align_call_ms"),
               kernel_ms=timings.get("kernel_ms"), genome_s=g.spent, report_s=t3 - t2 - g.spent, total_s=t3 - t0, pairs=int(idx.size),
               not_simple=int(((status != 0) & (status != a2i.ST_TIED)).sum()), blocks=timings["blocks"],
               host_blocks=timings["host_blocks"], host_blocks_s=timings["host_blocks_s"], detail_write_s=timings["detail_write_s"])
    if settle:
        out.update({key: timings[key] for key in ("settle_examined", "settle_settled", "settle_kernel_ms", "tied_rows")})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=100000)
    ap.add_argument("--mirnas", type=int, default=2000)
    ap.add_argument("--samples", type=int, default=8)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--record-runs", type=int, default=None)
    ap.add_argument("--settle-runs", type=int, default=None)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "a2i_report_timing.json"))
    args = ap.parse_args()
    record_runs = args.runs if args.record_runs is None else args.record_runs
    settle_runs = args.runs if args.settle_runs is None else args.settle_runs
    import torch
    from mirge_amd import a2i
    from mirge_amd.engine import Engine
    from mirge_amd.index import FmIndex
    eng = Engine(0)          # (raises without a GPU)
    t0 = time.time()
    w = synthesize(args.mirnas, args.reads, args.samples)
    eng.add_library("genome", FmIndex.build([w["genome"][0]], [w["genome"][1]]))
    genome = a2i.EngineGenome(eng, ["genome"])
    print("synthesised %d reads on %d miRNAs in %.1f s" % (args.reads, args.mirnas, time.time() - t0), flush=True)
    dev = {k: (None if w[k] is None else torch.from_numpy(w[k].view(np.int64) if k in ("words", "nmask") else w[k]).to(eng.device))
           for k in ("words", "nmask", "lens", "pass_id", "ref_id")}
    sample_list = ["s%d.fastq" % i for i in range(args.samples)]
    out = dict(what="annotate -ai: alignment of the miRNA reads to their miRNA and the three a2IEditing files", reads=args.reads,
               mirnas=args.mirnas, samples=args.samples, record_route=[], array_route=[],
               command="python scripts/a2i_report_timing.py " + " ".join(sys.argv[1:]))
    with tempfile.TemporaryDirectory() as d:
        a_dir, b_dir, c_dir = os.path.join(d, "a"), os.path.join(d, "b"), os.path.join(d, "c")
        os.mkdir(a_dir)
        os.mkdir(b_dir)
        os.mkdir(c_dir)
        array_route(w, dev, eng, genome, b_dir, sample_list, settle=True)    # warm-up: code objects
        for run in range(max(args.runs, record_runs)):
            if run < record_runs:
                r = record_route(w, genome, a_dir, sample_list)
                out["record_route"].append(r)
                print("run %d record route %.2f s" % (run, r["total_s"]), flush=True)
            if run >= args.runs:
                continue
            r = array_route(w, dev, eng, genome, b_dir, sample_list)
            out["array_route"].append(r)
            print("run %d array route %.3f s" % (run, r["total_s"]), flush=True)
        leg = dict(without=[], with_settle=[])
        for run in range(settle_runs):
            for key, flag, where in (("without", False, b_dir), ("with_settle", True, c_dir)):
                r = array_route(w, dev, eng, genome, where, sample_list, settle=flag)
                leg[key].append(r)
                print("run %d array route %s settle %.3f s, %d host blocks" % (run, "with" if flag else "without", r["total_s"],
                                                                               r["host_blocks"]), flush=True)
        same = True
        for fn in FILES:
            ref = open(os.path.join(b_dir, fn), "rb").read()
            same &= (not out["record_route"] or open(os.path.join(a_dir, fn), "rb").read() == ref)
            same &= (not settle_runs or open(os.path.join(c_dir, fn), "rb").read() == ref)
            out.setdefault("file_bytes", []).append(os.path.getsize(os.path.join(b_dir, fn)))
    old = [r["total_s"] for r in out["record_route"]]
    new = [r["total_s"] for r in out["array_route"]]
    out["files_equal"] = bool(same)
    out["record_fastest_s"], out["array_slowest_s"] = min(old), max(new)
    out["ratio_record_fastest_over_array_slowest"] = round(min(old) / max(new), 1)
    out["passed"] = bool(same and max(new) < min(old))
    if settle_runs:
        med = {key: float(np.median([r["total_s"] for r in runs])) for key, runs in leg.items()}
        leg.update(median_without_s=med["without"], median_with_settle_s=med["with_settle"],
                   ratio_without_over_with=round(med["without"] / med["with_settle"], 2),
                   fewer_host_blocks=bool(leg["with_settle"][0]["host_blocks"] < leg["without"][0]["host_blocks"]))
        out["settle_leg"] = leg
        out["passed"] = bool(out["passed"] and leg["fewer_host_blocks"])
    text = json.dumps(out)
    with open(args.json, "w") as fh:
        fh.write(text + "\n")
    print(text)
    return 0 if out["passed"] else 1


if __name__ == "__main__":
    sys.exit(main())
