#!/usr/bin/env python3
"""Capture tests/golden/trf_samples.json from the REFERENCE's own Python: the per-sample tRF reports of `-trf`
(writeDataToCSV.py :802-1088, `tRFs.samples.tmp/`) for two worlds, with the inputs to rerun them.

Run only in the build container.  Same scratch setup as make_golden.py, whose pieces it imports (a copy of the
reference outside the repository, CRLF stripped, lib2to3, the bowtie stand-in, stub_bio, PYTHONHASHSEED=2).  While
the reference runs, random.choice (W2C:708) is pinned to min as for trf.json, and the converted writeDataToCSV's
`np` is a proxy whose argsort is kind="stable" (min_distance's np.argsort(-rho), W2C:521, is not stable for large
float32 arrays in NumPy 2).

Worlds: "small" is build_trf_world(), the world of trf.json; "large" has the same libraries and tables and reads
drawn so that three tRNAs carry 200+ unique reads in clusters with halos and border densities, plus a one-row and
a two-row group (equal counts: a rho tie), a group without center, reads with N, overhanging trailer reads and a
trailer whose only reads overhang (an empty report block).

Stored per world: the sample list, quantStats, the trfContentDic that writeDataToCSV leaves at W2C:802 in its
order as (read index, tRNA index, start, tRF type index) rows -- counts and RPM follow from the reads and
quantStats as trf.write_trf_tables makes them, checked here --, the large world's (read, count per sample) rows,
and the eight files, zlib-compressed and base64-encoded.  Only data is written into the repository.
"""
import base64
import importlib
import json
import os
import random
import shutil
import subprocess
import sys
import tempfile
import types
import zlib

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402

ROOT = mg.ROOT
OUT = os.path.join(ROOT, "tests", "golden", "trf_samples.json")
SUFFIXES = (".potential_tRFs.report", ".potential_tRFs.summary.report", ".potential_tRFs.clusters.detail",
            ".tRFs.report.tsv")


def large_world_samples(libs, seed=907):
    """Reads of two samples over the tRNAs of build_trf_world(): sorted [read, count 0, count 1] rows."""
    import numpy as np
    rng = np.random.default_rng(seed)
    names, seqs = libs.libs["mature_trna"]
    pre_names, pre_seqs = libs.libs["pre_trna"]

    def mutate(r, ch=None):
        k = int(rng.integers(0, len(r)))
        c = ch if ch is not None else ("A" if r[k] != "A" else "G")
        return r[:k] + c + r[k + 1:]

    samples = []
    for si in range(2):
        reads = {}

        def put(r, c):
            reads[r] = reads.get(r, 0) + int(c)
        for t, n_uni in ((0, (300, 60)[si]), (5, (240, 50)[si]), (7, (210, 40)[si])):
            s = seqs[t]
            L = len(s)
            centers = [(0, 32), (0, 42), (L - 22, L), (33, L), (12, 40), (20, 52)]
            weight = [3000, 900, 2000, 700, 60, 25]
            uniq = set()
            while len(uniq) < n_uni:
                c = int(rng.integers(len(centers)))
                a, b = centers[c]
                if rng.random() < 0.1:                               # scattered reads: halos, far rows
                    a = int(rng.integers(0, L - 20))
                    b = int(rng.integers(a + 16, min(L, a + 45) + 1))
                a2 = min(max(a + int(rng.integers(-5, 6)), 0), L - 16)
                b2 = min(max(b + int(rng.integers(-5, 6)), a2 + 16), L)
                r = s[a2:b2]
                u = rng.random()
                if u < 0.3:
                    r = mutate(r)
                elif u < 0.36:
                    r = mutate(r, "N")
                exact = (a2, b2) == (a, b) and r == s[a:b]
                put(r, int(weight[c] * (0.5 + rng.random())) if exact else int(rng.zipf(1.6)) % 40 + 1)
                uniq.add(r)
        for k, m in enumerate(libs.libs["mirna"][1][:40]):            # miRNA reads (filter.py exits without)
            put(m[:22], 5 + 3 * k + si)
        put(seqs[8][0:30], 9)                                        # a one-row group
        put(seqs[9][0:25], 12)                                       # a two-row group, equal counts
        put(seqs[9][40:66], 12)
        for a in range(0, 52, 3):                                    # rho < 5 everywhere: no center, label -1
            put(seqs[6][a:a + 20], 1)
        for t in (0, 1):                                             # trailer reads, some overhanging
            s = pre_seqs[t]
            for a in (0, 2, 4, 6):
                ln = int(rng.integers(12, min(26, len(s) - a)))
                put(s[a:a + ln] + "T" * int(rng.integers(3, 6)), int(rng.integers(20, 300)))
            for a in (len(s) - 14, len(s) - 18):
                put(s[a:] + "T" * int(rng.integers(3, 6)), int(rng.integers(5, 60)))
        s = pre_seqs[5]                                              # a trailer with only overhanging reads
        for a in (len(s) - 13, len(s) - 15, len(s) - 20):
            put(s[a:] + "TTTT", int(rng.integers(2, 9)))
        samples.append({r: c for r, c in reads.items() if len(r) >= 16})
    return [[r] + [s.get(r, 0) for s in samples] for r in sorted(set(samples[0]) | set(samples[1]))]


def run_world(scratch, bindir, tag, libs, tables_txt, samples):
    """The reference's -trf path (quantReads -> runAnnotationPipeline -> summarize -> miRNAmerge -> filter ->
    writeDataToCSV) on one world: (trfContentDic rows at W2C:802, {file name: text})."""
    import numpy as real_np
    from mirge_amd import trf as my_trf
    RAP = importlib.import_module("mirge.utils.runAnnotationPipeline")
    W2C = importlib.import_module("mirge.utils.writeDataToCSV")
    from mirge.utils.quantReads import quantReads
    from mirge.utils.summarize import summarize
    from mirge.utils.miRNAmerge import miRNAmerge
    from mirge.utils.filter import filter as ref_filter

    libroot = os.path.join(scratch, "libs_" + tag)
    prefix = libs.write_layout(libroot, species="human", db="miRBase")
    for suffix, text in tables_txt.items():
        with open(os.path.join(libroot, "human", "annotation.Libs", "human" + suffix), "w") as fh:
            fh.write(text)
    t = my_trf.load_trf_tables(libroot, "human")
    outdir = os.path.join(scratch, "out_" + tag)
    os.makedirs(outdir)
    sample_list = ["t0.fastq", "t1.fastq"]
    seq_dic, len_dic = {}, {}
    for si, reads in enumerate(samples):
        fq = os.path.join(outdir, "t%d.trim.fastq" % si)
        with open(fq, "w") as fh:
            for k, r in enumerate(reads):
                fh.write("@r%d\n%s\n+\n%s\n" % (k, r, "I" * len(r)))
        quantReads(fq, seq_dic, len_dic, 2, si, sample_list, False, False)
    log_dic = {"quantStats": [{"filename": s} for s in sample_list], "annotStats": []}
    annot_names = ["exact miRNA", "hairpin miRNA", "mature tRNA", "primary tRNA", "snoRNA", "rRNA",
                   "ncrna others", "mRNA", "isomiR miRNA"]
    ix = lambda k: prefix + k
    trf_content = {}
    RAP.runAnnotationPipeline(bindir, seq_dic, "1", False, annot_names, outdir, log_dic,
                              ix("mirna_miRBase"), ix("hairpin_miRBase"), ix("mature_trna"), ix("pre_trna"),
                              ix("snorna"), ix("rrna"), ix("ncrna_others"), ix("mrna"), False, None, False,
                              None, None, "miRBase", True, t["trnaStruDic"], trf_content, sample_list)
    mir_dic, name_seq = {}, {}
    summarize(seq_dic, sample_list, log_dic, mir_dic, ix("mirna_miRBase"), outdir, False, bindir)
    miRNAmerge(os.path.join(libroot, "human", "annotation.Libs", "human_merges_miRBase.csv"), sample_list,
               mir_dic, os.path.join(libroot, "human", "fasta.Libs", "human_mirna_SNP_pseudo_miRBase.fa"), name_seq)
    ref_filter(mir_dic, sample_list, log_dic, "0.1")
    merged_name = {}
    for line in libs.merges:
        f = line.split(",")
        for m in f[1:]:
            merged_name[m] = f[0]
    stable = types.SimpleNamespace(**{k: getattr(real_np, k) for k in dir(real_np) if not k.startswith("__")})
    stable.argsort = lambda a, *args, **kw: real_np.argsort(a, kind="stable")
    real_choice, W2C.np = random.choice, stable
    random.choice = lambda seq: min(seq)
    try:
        W2C.writeDataToCSV(outdir, annot_names, sample_list, False, False, log_dic, seq_dic, mir_dic, name_seq,
                           merged_name, bindir, None, "1", False, [], False, False, None, "miRBase", True,
                           trf_content, t["trnaStruDic"], ix("pre_trna"), t["duptRNA2UniqueDic"],
                           t["trnaAAanticodonDic"], t["tRNAtrfDic"], t["trfMergedNameDic"], t["trfMergedList"])
    finally:
        random.choice, W2C.np = real_choice, real_np
    quant_stats = [{k: v for k, v in q.items() if k != "filename"} for q in log_dic["quantStats"]]
    return trf_content, quant_stats, outdir, sample_list


def table(world, trf_content, quant_stats, reads):
    """trfContentDic rows as indices; the counts and RPM it holds must follow from `reads` and quantStats."""
    index = {r[0]: k for k, r in enumerate(reads)}
    names, types_, rows = [], [], []
    for read, rec in trf_content.items():
        (name,) = [k for k in rec if k not in ("uid", "RPM", "count")]
        counts = reads[index[read]][1:]
        assert rec["count"] == counts
        for i, q in enumerate(quant_stats):
            d = q["maturetrnaReads"] + q["pretrnaReads"]
            assert rec["RPM"][i] == (100000.0 * counts[i] / d if d else 0.0)
        e = rec[name]
        for lst, v in ((names, name), (types_, e["tRFType"])):
            if v not in lst:
                lst.append(v)
        rows.append([index[read], names.index(name), e["start"], types_.index(e["tRFType"])])
    world.update(quantStats=quant_stats, trf_names=names, trf_types=types_, trfContentDic=rows)


def files_of(outdir, sample_list):
    files = {}
    for s in sample_list:
        for suf in SUFFIXES:
            files[s + suf] = open(os.path.join(outdir, "tRFs.samples.tmp", s + suf)).read()
    return {k: base64.b64encode(zlib.compress(v.encode(), 9)).decode() for k, v in sorted(files.items())}


def main():
    if os.environ.get("PYTHONHASHSEED") != "2":
        env = dict(os.environ, PYTHONHASHSEED="2")
        sys.exit(subprocess.run([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env).returncode)
    scratch = tempfile.mkdtemp(prefix="mirge_golden_trfs_")
    try:
        pkg = os.path.join(scratch, "mirge")
        shutil.copytree(mg.REF, pkg)
        subprocess.run(["chmod", "-R", "u+w", pkg], check=True)
        for dp, _, fns in os.walk(pkg):
            for fn in fns:
                if fn.endswith(".py"):
                    p = os.path.join(dp, fn)
                    data = open(p, "rb").read().replace(b"\r\n", b"\n")
                    open(p, "wb").write(data)
        subprocess.run([sys.executable, "-m", "lib2to3", "-w", "-n"] +
                       [os.path.join(pkg, "utils", m + ".py") for m in mg.HOT],
                       check=True, capture_output=True)
        bindir = os.path.join(scratch, "bin")
        os.makedirs(bindir)
        for prog in ("bowtie", "bowtie-inspect"):
            p = os.path.join(bindir, prog)
            open(p, "w").write(mg.BOWTIE_STANDIN % {"root": ROOT})
            os.chmod(p, 0o755)
        mg.stub_bio()
        sys.path.insert(0, scratch)

        libs, tables_txt, samples = mg.build_trf_world()
        with open(os.path.join(ROOT, "tests", "golden", "trf.json")) as fh:
            small = json.load(fh)
        assert samples == small["samples"] and tables_txt == small["tables"], "build_trf_world() is not trf.json's"
        worlds = {}
        for tag in ("small", "large"):
            if tag == "small":
                reads = [[r, samples[0].count(r), samples[1].count(r)] for r in sorted(set(samples[0] + samples[1]))]
                w, run = {"reads_from": "trf.json"}, samples
            else:
                reads = large_world_samples(libs)
                w = {"reads": reads}
                run = [[r[0] for r in reads for _ in range(r[1 + i])] for i in range(2)]
            content, qs, outdir, sample_list = run_world(scratch, bindir, tag, libs, tables_txt, run)
            table(w, content, qs, reads)
            w.update(sample_list=sample_list, files_z=files_of(outdir, sample_list))
            worlds[tag] = w
        golden = {
            "about": "captured from the reference's Python (-trf, W2C:802-1088) by "
                     "tests/golden/make_golden_trf_samples.py; bowtie is the stand-in, random.choice pinned to "
                     "min, writeDataToCSV's np.argsort swapped for kind='stable' (the pinned rank order)",
            "worlds": worlds,
        }
        with open(OUT, "w") as fh:
            json.dump(golden, fh, separators=(",", ":"), sort_keys=True)
        for k, w in worlds.items():
            print(k, "tRF reads", len(w["trfContentDic"]))
        print("wrote", OUT, os.path.getsize(OUT), "bytes")
    finally:
        shutil.rmtree(scratch, ignore_errors=True)


if __name__ == "__main__":
    main()
