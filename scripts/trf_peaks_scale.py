#!/usr/bin/env python3
"""Density peaks of `-trf` at scale: 8 samples x 400 tRNAs with heavy-tailed group sizes (largest 20 000 rows,
about 10^6 rows in all) through mirge_amd.trf_samples.run_peaks on the GPU.  Times the three launches with HIP
events and the host part separately; prints one JSON line with sum n^2 and pairs per second."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def group_sizes(n_groups, largest, total):
    """largest * k^-a for k = 1..n_groups, a chosen by bisection so that they add up to about `total`."""
    k, lo, hi = np.arange(1, n_groups + 1, dtype=np.float64), 0.0, 4.0
    for _ in range(60):
        a = (lo + hi) / 2
        lo, hi = (a, hi) if np.maximum(1, np.floor(largest * k ** -a)).sum() > total else (lo, a)
    return np.maximum(1, np.floor(largest * k ** -a)).astype(np.int64)


def synth_group(n, rng, L=76):
    """Reads around five fragments of one template (+-5 at both ends), 30 % with a substitution or N."""
    from mirge_amd.trf_samples import Group
    tmpl = rng.choice(np.frombuffer(b"ACGT", np.uint8), L)
    centers = np.array([(0, 32), (0, 42), (L - 22, L), (33, L), (12, 40)])[rng.integers(0, 5, n)]
    a = np.clip(centers[:, 0] + rng.integers(-5, 6, n), 0, L - 16)
    b = np.clip(centers[:, 1] + rng.integers(-5, 6, n), a + 16, L)
    pos = np.arange(L)[None, :]
    m = np.where((pos >= a[:, None]) & (pos < b[:, None]), tmpl[None, :], ord("-")).astype(np.uint8)
    mut = np.nonzero(rng.random(n) < 0.3)[0]
    m[mut, np.minimum(a[mut] + rng.integers(0, 16, len(mut)), L - 1)] = rng.choice(np.frombuffer(b"ACGTN", np.uint8), len(mut))
    rpm = [float("%.3f" % x) for x in rng.pareto(1.2, n) + 0.5]
    return Group([(bytes(r).decode(), "x", 1, x) for r, x in zip(m, rpm)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=8 * 400)
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--largest", type=int, default=20000)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    import torch
    from mirge_amd import trf_samples
    from mirge_amd.engine import Engine
    rng = np.random.default_rng(5)
    sizes = group_sizes(args.groups, args.largest, args.rows)
    rng.shuffle(sizes)
    t0 = time.perf_counter()
    groups = [synth_group(int(n), rng) for n in sizes]
    t_build = time.perf_counter() - t0
    eng = Engine(0)
    runs = []
    for _ in range(args.reps + 1):               # the first is a warm-up
        ms, wall = {}, [0.0]

        def timed(key, fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t = time.perf_counter()
            e0.record()
            out = fn()
            e1.record()
            e1.synchronize()
            wall[0] += time.perf_counter() - t
            ms[key] = e0.elapsed_time(e1)
            return out

        def peaks(*a):
            st = timed("rho", lambda: eng.trf_peaks(*a))
            md, bo = st.min_distance, st.border
            st.min_distance = lambda r: timed("delta", lambda: md(r))
            st.border = lambda lab, off: timed("border", lambda: bo(lab, off))
            return st
        t = time.perf_counter()
        trf_samples.run_peaks(groups, peaks)
        runs.append(dict(ms, host_s=time.perf_counter() - t - wall[0]))
    med = {k: float(np.median([r.get(k, 0.0) for r in runs[1:]])) for k in ("rho", "delta", "border", "host_s")}
    pairs = int((sizes ** 2).sum())
    print(json.dumps(dict(
        metric="trf_peaks_scale", groups=len(sizes), rows=int(sizes.sum()), largest=int(sizes.max()), sum_n2=pairs,
        rho_ms=round(med["rho"], 3), delta_ms=round(med["delta"], 3), border_ms=round(med["border"], 3),
        gpu_ms=round(med["rho"] + med["delta"] + med["border"], 3), rho_pairs_per_s=round(pairs / med["rho"] * 1e3, 1),
        host_run_peaks_s=round(med["host_s"], 3), host_group_build_s=round(t_build, 3), reps=args.reps,
        device=eng.arch)))


if __name__ == "__main__":
    main()
