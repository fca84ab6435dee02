#!/usr/bin/env python3
"""Host builder against the device route of the index builder (csrc/sa_build.hip) on synthetic texts.
    python scripts/index_build_timing.py [--sizes 1,32,137,300] [--runs 3] [--out profiles/index_build_device.json]
Sizes are in Mbp.  137 is the synthetic mRNA library of mirge_amd.synth at full scale; every other size is uniform
random bases with twenty copies of one block (200 kb, or 1/160 of a text below 32 Mbp) planted in it, cut into entries
of 1 Mbp.  Every (size, route) pair runs in a child process of its own under a time limit; the parent never opens the
GPU.  A child times the C-ABI call alone (the entries are encoded before the clock starts), `--runs` times, and passes
on the stage laps of the device route (MIRGE_AMD_TIMING).  Results are merged into the JSON file by size."""
import argparse
import ctypes as C
import json
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LIMIT_S = {"host": 900, "device": 300}


def make_text(mbp):
    import numpy as np
    if mbp == 137:
        from mirge_amd import synth
        names, seqs = synth.SynthLibraries(seed=20181, scale=1.0).libs["mrna"]
        return list(names), list(seqs)
    n = int(mbp) * 1000000
    rng = np.random.default_rng(1000 + int(mbp))
    codes = rng.integers(0, 4, n, dtype=np.uint8)
    block = min(200000, n // 160)
    src = codes[:block].copy()
    for at in rng.integers(block, n - block, 20):
        codes[int(at):int(at) + block] = src
    text = np.frombuffer(b"ACGT", dtype=np.uint8)[codes].tobytes()
    seqs = [text[o:o + 1000000] for o in range(0, n, 1000000)]
    return ["e%d" % i for i in range(len(seqs))], seqs


def child(mbp, route, runs):
    if route == "device":
        os.environ["MIRGE_AMD_TIMING"] = "1"
    from mirge_amd import _native
    lib = _native.load()
    names, seqs = make_text(mbp)
    n = len(names)
    arr_n = (C.c_char_p * n)(*[s.encode("ascii") for s in names])
    arr_s = (C.c_char_p * n)(*[s if isinstance(s, bytes) else s.encode("ascii") for s in seqs])
    bases = sum(len(s) for s in seqs)
    times, rounds = [], None
    for r in range(runs):
        h = C.c_void_p()
        sys.stderr.write("[run] %d\n" % r)
        sys.stderr.flush()
        t0 = time.perf_counter()
        if route == "device":
            rc = lib.mrg_index_build_device(0, arr_n, arr_s, n, C.byref(h))
        else:
            rc = lib.mrg_index_build(arr_n, arr_s, n, C.byref(h))
        times.append(time.perf_counter() - t0)
        _native.check(rc)
        if route == "device":
            rounds = int(lib.mrg_index_build_device_rounds())
        lib.mrg_index_free(h)
    print(json.dumps(dict(bases=bases, entries=n, seconds=times, rounds=rounds)))


def laps_of(stderr_text):
    """[{stage: seconds}] per run, from the `[timing] build_index (device): <stage> <s> s` lines"""
    runs, cur = [], None
    for line in stderr_text.splitlines():
        if line.startswith("[run]"):
            cur = {}
            runs.append(cur)
            continue
        m = re.match(r"\[timing\] build_index \(device\): (.*) ([0-9.]+) s$", line)
        if m and cur is not None:
            stage = m.group(1)
            stage = "sort rounds" if stage.startswith("sort round") else stage
            cur[stage] = round(cur.get(stage, 0.0) + float(m.group(2)), 4)
    return runs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1,32,137,300")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "index_build_device.json"))
    ap.add_argument("--child", nargs=2, metavar=("MBP", "ROUTE"))
    args = ap.parse_args()
    if args.child:
        return child(int(args.child[0]), args.child[1], args.runs)
    result = {}
    if os.path.isfile(args.out):
        with open(args.out) as fh:
            result = json.load(fh)
    for mbp in [int(s) for s in args.sizes.split(",")]:
        row = {}
        for route in ("device", "host"):
            t0 = time.time()
            try:
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(mbp), route, "--runs", str(args.runs)],
                                   capture_output=True, text=True, timeout=LIMIT_S[route])
            except subprocess.TimeoutExpired:
                print("%d Mbp %s: no answer within %d s; stopping" % (mbp, route, LIMIT_S[route]), file=sys.stderr)
                return 1
            if p.returncode != 0:
                print("%d Mbp %s: exit status %d; stopping\n%s" % (mbp, route, p.returncode, p.stderr[-2000:]), file=sys.stderr)
                return 1
            r = json.loads(p.stdout.strip().splitlines()[-1])
            s = r["seconds"]
            row["bases"], row["entries"] = r["bases"], r["entries"]
            row[route] = dict(seconds=[round(x, 4) for x in s], min=round(min(s), 4), max=round(max(s), 4))
            if route == "device":
                row[route]["rounds"] = r["rounds"]
                row[route]["laps"] = laps_of(p.stderr)
            print("%d Mbp %s: min %.3f s, max %.3f s (%d runs; %.0f s with the text)" % (mbp, route, min(s), max(s), len(s), time.time() - t0),
                  flush=True)
        row["host_min_over_device_max"] = round(row["host"]["min"] / row["device"]["max"], 2)
        row["device_slowest_beats_host_fastest"] = row["device"]["max"] < row["host"]["min"]
        result[str(mbp)] = row
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1, sort_keys=True)
            fh.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
