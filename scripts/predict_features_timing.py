#!/usr/bin/env python3
"""Timing of predict mode's cluster feature table (miRge2.0.py:604) on a world made as scripts/predict_cluster_timing.py
makes its own (a seeded synthetic genome of --parts parts of --part-bases bases, --reads collapsed reads), with the read
piles deepened: one locus per --reads-per-locus reads and a jitter of +-4, so that the clusters stay within 32 nt and most
of them hold three members and a count sum of 10; plus one locus with --deep reads whose four cut bases vary, which pass 2
all lists on one cluster: the single-wave walk of the largest group.  Both laps start at the return of the remap writer, i.e.
with `*_vs_representative_seq_modified_selected_sorted.tsv` on disk and the reads, the trim's arrays and the rows where that
stage left them:

  (a) the Python model over the table's text (tests/predict_features_model.run: a2i.local_pair per line, lists of strings);
  (b) predict.cluster_features to the last byte of both files.

Each route runs once as a warm-up and then --runs times in this one process; the files of the two routes must be equal.  No
ratio is fixed in advance.  Writes one JSON object to --json, default profiles/predict_features_timing.json, and prints it."""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402


def spread(xs):
    return dict(min=round(min(xs), 6), max=round(max(xs), 6))


def synthesize(d, parts, part_bases, n_reads, per_locus, deep):
    from mirge_amd.index import FmIndex
    rng = np.random.default_rng(604)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    texts = []
    for k in range(parts):
        t = acgt[rng.integers(0, 4, part_bases)].tobytes()
        texts.append(t)
        FmIndex.build(["chr%d" % (k + 1)], [t.decode()]).save(os.path.join(d, "g.part%03d.mrgfm" % k))
    loci = rng.integers(1000, part_bases - 1000, max(1, n_reads // per_locus))
    loci_p = rng.integers(0, parts, loci.size)
    comp = bytes.maketrans(b"ACGT", b"TGCA")
    seen, lines = set(), []

    def add(q):
        if q not in seen:
            seen.add(q)
            lines.append(b">mir%d_%d\n%s\n" % (len(lines), 1 + len(lines) % 211, q))
    while len(lines) < n_reads:
        L = int(rng.integers(18, 24))
        if rng.random() < 0.9:
            i = int(rng.integers(0, loci.size))
            at = int(loci[i]) + int(rng.integers(-4, 5))
            q = bytearray(texts[int(loci_p[i])][at:at + L])
            if rng.random() < 0.3:
                j = int(rng.integers(0, L))
                q[j] = b"ACGT"[(b"ACGT".index(q[j]) + 1) % 4]
            q = bytes(q)
            if i % 2:
                q = q[::-1].translate(comp)
        else:
            q = acgt[rng.integers(0, 4, L)].tobytes()
        add(q)
    # the deep pile: exact reads that make the cluster, then reads whose first base and last three vary (pass 2 cuts them)
    at = int(rng.integers(1000, part_bases - 1000))
    for off in range(-4, 5):
        for L in range(18, 24):
            add(texts[0][at + off:at + off + L])
    if deep > 9 * 8 * 256 // 2:   # (offsets x lengths x cut bases: drawing more distinct reads than half of them would crawl)
        raise SystemExit("--deep: at most %d distinct reads can be cut at one locus this way" % (9 * 8 * 256 // 2))
    want = len(lines) + deep
    while len(lines) < want:
        L = int(rng.integers(18, 26))
        off = int(rng.integers(-4, 5))
        q = bytearray(texts[0][at + off:at + off + L])
        q[0] = acgt[rng.integers(0, 4)]
        q[L - 3:L] = acgt[rng.integers(0, 4, 3)].tobytes()
        add(bytes(q))
    with open(os.path.join(d, "reads.fa"), "wb") as fh:
        fh.write(b"".join(lines))
    return {"chr%d" % (k + 1): t.decode() for k, t in enumerate(texts)}


def largest_group_walk(eng, rs, counts, res, kept_seq_off, runs):
    """Wall time (device events) of mrg_predict_feature_tally over the largest tallied group alone: one wave."""
    import torch
    ok = (res["group_pass"] != 0) & (res["group_host"] == 0)
    if not ok.any():
        return None
    sizes = np.diff(res["group_off"].astype(np.int64))
    g = int(np.argmax(np.where(ok, sizes, 0)))
    lo, hi = int(res["group_off"][g]), int(res["group_off"][g + 1])
    c = int(res["group_cluster"][g])
    dev = eng.device
    up = lambda a, dt, view=None: torch.from_numpy(np.ascontiguousarray(a, dtype=dt).view(view or dt)).to(dev)
    ins = [up([0, hi - lo], np.uint32, np.int32), up([0], np.uint32, np.int32), up([1], np.uint8), up([0], np.uint8),
           up(res["row_read"][lo:hi], np.uint32, np.int32), up(res["row_diag"][lo:hi], np.int32), up(res["row_ident"][lo:hi], np.uint8),
           eng._dev_u32(counts), up([int(kept_seq_off[c + 1] - kept_seq_off[c])], np.uint8)]
    outs = [torch.zeros(8, dtype=torch.uint8, device=dev), torch.zeros(8, dtype=torch.int32, device=dev),
            torch.zeros(8, dtype=torch.int64, device=dev), torch.zeros(64, dtype=torch.int64, device=dev)]
    laps = []
    for k in range(runs + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(torch.cuda.current_stream(dev))
        rc = eng._lib.mrg_predict_feature_tally(
            eng._h, 1, ins[0].data_ptr(), ins[1].data_ptr(), ins[2].data_ptr(), ins[3].data_ptr(), hi - lo, ins[4].data_ptr(), ins[5].data_ptr(),
            ins[6].data_ptr(), rs.words.data_ptr(), rs.lens.data_ptr(), rs.n, ins[7].data_ptr(), 1, ins[8].data_ptr(), outs[0].data_ptr(),
            outs[1].data_ptr(), outs[2].data_ptr(), outs[3].data_ptr(), eng._stream_ptr())
        assert rc == 0
        b.record(torch.cuda.current_stream(dev))
        b.synchronize()
        if k:
            laps.append(a.elapsed_time(b))
    assert tuple(outs[1].cpu().numpy()[:4]) == tuple(res["frame"][g])
    return dict(members=hi - lo, tally_ms=spread(laps))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", type=int, default=2)
    ap.add_argument("--part-bases", type=int, default=20_000_000)
    ap.add_argument("--reads", type=int, default=120_000)
    ap.add_argument("--reads-per-locus", type=int, default=10)
    ap.add_argument("--deep", type=int, default=8_000)
    ap.add_argument("--cutoff", type=int, default=30)
    ap.add_argument("--seed-length", type=int, default=25)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "predict_features_timing.json"))
    args = ap.parse_args()
    import predict_cluster_timing as world
    from mirge_amd import predict
    from mirge_amd.engine import STRATUM_ALL
    from tests import predict_features_model as model
    with tempfile.TemporaryDirectory() as d:
        t0 = time.time()
        chromosomes = synthesize(d, args.parts, args.part_bases, args.reads, args.reads_per_locus, args.deep)
        res = dict(what="predict mode: the cluster feature table", parts=args.parts, part_bases=args.part_bases, reads=args.reads,
                   reads_per_locus=args.reads_per_locus, deep=args.deep, cutoff=args.cutoff, seed_length=args.seed_length, runs=args.runs,
                   synthesis_and_index_build_s=round(time.time() - t0, 1))
        eng, parts, keys, names, seqs, rs = world.open_world(d)
        counts = predict.read_counts(names)
        numbers = predict.read_numbers(names)
        keep = np.array(["chr" in nm for ix in parts for nm in ix.names], dtype=bool)
        cl = eng.cluster_valid(rs, keys, counts, entry_keep=keep, threshold=14, strands=2, stratum_mode=STRATUM_ALL, m=3, seed_len=25,
                               max_mm_seed=0, max_mm_total=2, keep_device=True)
        out_stem = os.path.join(d, "unmapped_mirna_smp")
        predict.write_clusters(out_stem + "_vs_genome_sorted_clusters.tsv", predict.sample_name(out_stem + "_vs_genome_sorted.sam"), parts,
                               names, cl)
        tr = predict.trim_clusters(eng, cl, predict.load_repeats(None, parts), args.cutoff, out_stem, names)
        tr = dict(tr, clusters=predict.retained_clusters(cl, tr))
        remap = predict.map_reads_to_clusters(eng, rs, numbers, counts, tr, args.seed_length, out_stem, keep_device=True)
        table = out_stem + predict.REMAP_SUFFIX
        res.update(clusters=len(cl["entry"]), retained=tr["n_retained"], rows=remap["n_rows"], table_bytes=os.path.getsize(table))
        # (b): one call ahead of the laps pays the kernels' first use
        laps = []
        for k in range(args.runs + 1):
            tm = {}
            t = time.perf_counter()
            got = predict.cluster_features(eng, rs, counts, tr, remap, parts, out_stem, timings=tm)
            print("# route b, lap %d: %.3f s" % (k, time.perf_counter() - t), file=sys.stderr, flush=True)
            if k:
                laps.append(dict(total_s=time.perf_counter() - t, device_ms=tm["device_ms"], download_ms=tm["download_ms"], host_s=tm["host_s"],
                                 write_s=tm["write_s"]))
        res["b_array_route"] = {k: spread([lap[k] for lap in laps]) for k in laps[0]}
        res["b_writer_share"] = spread([lap["write_s"] / lap["total_s"] for lap in laps])
        res["b_host_group_share"] = spread([lap["host_s"] / lap["total_s"] for lap in laps])
        res.update(groups=got["seen"], groups_passed=got["passed"], groups_written=got["written"], feature_lines=got["lines"],
                   host_groups=got["host_groups"], row_status_counts=[int(x) for x in got["row_status_counts"]])
        res["largest_group"] = largest_group_walk(eng, rs, counts, got, np.asarray(tr["kept_seq_off"]), args.runs)
        files_b = [open(table[:-4] + s, "rb").read() for s in (predict.FEATURES_SUFFIX, predict.CLUSTER_SUFFIX)]
        res["features_bytes"], res["cluster_bytes"] = len(files_b[0]), len(files_b[1])
        eng.close()
        print("# %d groups, %d pass the filter, %d on the host" % (got["seen"], got["passed"], got["host_groups"]), file=sys.stderr, flush=True)
        # (a) the model over the table's text
        laps = []
        for k in range(args.runs + 1):
            t = time.perf_counter()
            text = open(table).read()
            feats, clus, _ = model.run(text, chromosomes, os.path.basename(table))
            for s, body in ((predict.FEATURES_SUFFIX, feats), (predict.CLUSTER_SUFFIX, clus)):
                with open(os.path.join(d, "a" + s), "w") as fh:
                    fh.write(body)
            print("# route a, lap %d: %.1f s" % (k, time.perf_counter() - t), file=sys.stderr, flush=True)
            if k:
                laps.append(time.perf_counter() - t)
        res["a_model_route_s"] = spread(laps)
        res["files_equal"] = [feats.encode(), clus.encode()] == files_b
        assert res["files_equal"], "the two routes' files differ"
    a, b = res["a_model_route_s"], res["b_array_route"]["total_s"]
    res["ratio_b_over_a"] = dict(best=round(b["min"] / a["max"], 5), worst=round(b["max"] / a["min"], 5))
    res["command"] = "python scripts/predict_features_timing.py --parts %d --part-bases %d --reads %d --reads-per-locus %d --deep %d" % (
        args.parts, args.part_bases, args.reads, args.reads_per_locus, args.deep)
    out = json.dumps(res)
    with open(args.json, "w") as fh:
        fh.write(out + "\n")
    print(out)


if __name__ == "__main__":
    main()
