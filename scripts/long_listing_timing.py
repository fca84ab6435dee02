#!/usr/bin/env python3
"""Timing of the ragged listing next to the packed one (a record, not a gate): --reads reads of --long-len nt through
Engine.list_valid_long (long_valid_kernel, one wave per read) and as many reads of --short-len nt, drawn the same way,
through Engine.list_valid (valid_kernel, one lane per read), in the same process against one synthetic part of
--part-bases random bases; policy `-n 0 -l 25 -a`, both strands.  80 % of the reads are cut from the part with 0-1
substitutions on either strand, the rest are random.  Each listing runs --warmup times untimed, then the two alternate
--repeats times; the figures are the count and fill sweeps' synchronised wall seconds (median and minimum) and the
ratio of the medians.  Prints one JSON line and, with --out, writes it to that file."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np


def draw(rng, text, n, L):
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    seqs = []
    for _ in range(n):
        if rng.random() < 0.8:
            at = int(rng.integers(0, len(text) - L))
            q = text[at:at + L].decode()
            if rng.random() < 0.3:
                i = int(rng.integers(0, L))
                q = q[:i] + "ACGT"[("ACGT".index(q[i]) + 1) % 4] + q[i + 1:]
            if rng.random() < 0.5:
                q = q[::-1].translate(str.maketrans("ACGT", "TGCA"))
        else:
            q = acgt[rng.integers(0, 4, L)].tobytes().decode()
        seqs.append(q)
    return seqs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part-bases", type=int, default=20_000_000)
    ap.add_argument("--reads", type=int, default=1000)
    ap.add_argument("--long-len", type=int, default=300)
    ap.add_argument("--short-len", type=int, default=255)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=11)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from mirge_amd import pack
    from mirge_amd.engine import Engine, ReadSet, STRATUM_ALL
    from mirge_amd.index import FmIndex
    rng = np.random.default_rng(818)
    text = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, args.part_bases)].tobytes()
    eng = Engine(int(os.environ.get("MIRGE_AMD_GPU", "0")))
    eng.add_library("part", FmIndex.build(["chr1"], [text.decode()]), exact_dict=False)
    long_reads, short_reads = draw(rng, text, args.reads, args.long_len), draw(rng, text, args.reads, args.short_len)
    rs = ReadSet(*pack.pack_reads(short_reads), device=eng.device)
    how = dict(strands=2, stratum_mode=STRATUM_ALL, seed_len=25, max_mm_seed=0, max_mm_total=2)

    def run_long(tm):
        return eng.list_valid_long(long_reads, ["part"], timings=tm, **how)

    def run_short(tm):
        return eng.list_valid(rs, ["part"], timings=tm, **how)
    times = {"long": [], "short": []}
    rows = {}
    for i in range(args.warmup + args.repeats):
        for name, fn in (("long", run_long), ("short", run_short)):
            tm = {}
            rows[name] = int(fn(tm)[0][-1])
            if i >= args.warmup:
                times[name].append((tm["count_s"], tm["fill_s"]))
    eng.close()
    out = dict(what="ragged listing next to the packed listing, -n 0 -l 25 -a, both strands", part_bases=args.part_bases,
               reads=args.reads, repeats=args.repeats)
    for name, L in (("long", args.long_len), ("short", args.short_len)):
        total = [c + f for c, f in times[name]]
        out[name] = dict(read_len=L, rows=rows[name], count_s_median=statistics.median(c for c, _ in times[name]),
                         fill_s_median=statistics.median(f for _, f in times[name]), total_s_median=statistics.median(total),
                         total_s_min=min(total))
    out["ratio_long_over_short"] = out["long"]["total_s_median"] / out["short"]["total_s_median"]
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
