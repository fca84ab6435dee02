#!/usr/bin/env python3
"""Timing of the bowtie front end on predict mode's genome call (miRge2.0.py:538: `-f -n 0 -m 3 -l 25 -S -a --best`):
--reads unique 16-25 nt reads (80 % cut from the genome with 0-1 substitutions, either strand; the rest random)
against a synthetic genome of --parts parts of --part-bases random bases, each its own `.partNNN.mrgfm` library.
Runs the front end's own path in-process (Engine.list_valid + mrg_write_bowtie, as mirge_amd.bowtie.align) and
prints one JSON line: seconds from start to libraries resident (synthesis, index build, upload), the count and fill
sweeps (synchronised wall time), the writer's time and bytes.  Default = 3 Gbp in 500 Mbp parts, 10^6 reads."""
import argparse
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", type=int, default=6)
    ap.add_argument("--part-bases", type=int, default=500_000_000)
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--out", default=None, help="SAM path (default: a temporary file, removed)")
    args = ap.parse_args()
    from mirge_amd import bowtie, pack
    from mirge_amd.engine import Engine, ReadSet, STRATUM_ALL
    from mirge_amd.index import FmIndex
    t0 = time.time()
    rng = np.random.default_rng(538)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    eng = Engine(int(os.environ.get("MIRGE_AMD_GPU", "0")))
    parts, keys, texts = [], [], []
    for k in range(args.parts):
        t = acgt[rng.integers(0, 4, args.part_bases)].tobytes()
        texts.append(t)
        ix = FmIndex.build(["chr%d" % (k + 1)], [t.decode()])
        keys.append("part%03d" % k)
        eng.add_library(keys[-1], ix, exact_dict=False)
        parts.append(ix)
    t_resident = time.time() - t0
    seqs, seen = [], set()
    while len(seqs) < args.reads:
        L = int(rng.integers(16, 26))
        if rng.random() < 0.8:
            t = texts[int(rng.integers(0, args.parts))]
            at = int(rng.integers(0, args.part_bases - L))
            q = t[at:at + L].decode()
            if rng.random() < 0.3:
                i = int(rng.integers(0, L))
                q = q[:i] + "ACGT"[("ACGT".index(q[i]) + 1) % 4] + q[i + 1:]
            if rng.random() < 0.5:
                q = q[::-1].translate(str.maketrans("ACGT", "TGCA"))
        else:
            q = acgt[rng.integers(0, 4, L)].tobytes().decode()
        if q not in seen:
            seen.add(q)
            seqs.append(q)
    del texts, seen
    words, lens, nmask = pack.pack_reads(seqs, 1)
    rs = ReadSet(words, lens, nmask, device=eng.device)
    tm = {}
    t1 = time.time()
    off, entry, offset, strand, mm, supp = eng.list_valid(rs, keys, strands=2, stratum_mode=STRATUM_ALL, m=3, seed_len=25,
                                                          max_mm_seed=0, max_mm_total=2, timings=tm)
    t_list = time.time() - t1
    fd, path = (None, args.out) if args.out else tempfile.mkstemp(suffix=".sam")
    if fd is not None:
        os.close(fd)
    names = ["r%d" % i for i in range(len(seqs))]
    t2 = time.time()
    s = bowtie.write_bowtie(path, True, "bowtie -f -n 0 -m 3 -l 25 -S -a --best genome reads.fa", parts, names, seqs, off, entry,
                            offset, strand, mm, supp, 3)
    t_write = time.time() - t2
    size = os.path.getsize(path)
    if not args.out:
        os.remove(path)
    eng.close()
    print(json.dumps(dict(what="bowtie shim, predict genome call", parts=args.parts, part_bases=args.part_bases,
                          reads=len(seqs), s_to_resident=round(t_resident, 2), count_sweeps_s=round(tm["count_s"], 4),
                          fill_sweeps_s=round(tm["fill_s"], 4), list_valid_total_s=round(t_list, 3),
                          writer_s=round(t_write, 3), bytes_written=size, alignments=s["reported"], aligned=s["aligned"],
                          suppressed=s["suppressed"])))


if __name__ == "__main__":
    main()
