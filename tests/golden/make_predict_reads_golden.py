#!/usr/bin/env python3
"""Capture tests/golden/predict_reads.json from the REFERENCE's own convert2Fasta (utils/convert2Fasta.py): seeded
unmapped.csv texts and every file it writes for them.

    python tests/golden/make_predict_reads_golden.py <reference src/mirge directory>

Run only in the build container: the one module is copied to a scratch directory outside the
repository, CRLF stripped, and imported from there.  Only data is written into the repository: per case the parameters, the
CSV text and the text of every file.

Cases: S = 1, 2, 3 with and without the spike-in column (startP 12 / 11); lengths 15, 16, 25, 26 and between; cutoffs 1, 2
and 5; a window with min == max; zero counts; a read whose samples are each below the cutoff while the sum reaches it;
reads with N; two samples with one stem; an empty table.
"""
import importlib.util
import json
import os
import shutil
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "predict_reads.json")
NAMES = ["exact miRNA", "hairpin miRNA", "mature tRNA", "primary tRNA", "snoRNA", "rRNA", "ncrna others", "mRNA", "isomiR miRNA"]


def load_reference(src):
    tmp = tempfile.mkdtemp(prefix="predict_reads_golden_")
    dst = os.path.join(tmp, "convert2Fasta.py")
    shutil.copy(os.path.join(src, "utils", "convert2Fasta.py"), dst)
    os.chmod(dst, 0o644)
    with open(dst, "rb") as fh:
        data = fh.read().replace(b"\r\n", b"\n")
    with open(dst, "wb") as fh:
        fh.write(data)
    spec = importlib.util.spec_from_file_location("convert2Fasta", dst)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return tmp, mod.convert2Fasta


def csv_text(samples, seqs, quant, spike):
    names = NAMES + (["spike-in"] if spike else [])
    rows = ["uniqueSequence,annotFlag," + ",".join(names) + "," + ",".join(samples) + "\n"]
    for seq, q in zip(seqs, quant):
        rows.append("%s,0,%s,%s\n" % (seq, "," * (len(names) - 1), ",".join(str(x) for x in q)))
    return "".join(rows)


def world(seed, S, n=36):
    rng = np.random.default_rng(seed)
    seqs, seen = [], set()
    while len(seqs) < n:
        L = int(rng.choice([15, 16, 16, 17, 20, 20, 22, 25, 25, 26, 31]))
        s = "".join("ACGTN"[c] for c in rng.choice(5, L, p=[0.245] * 4 + [0.02]))
        if s not in seen:
            seen.add(s)
            seqs.append(s)
    quant = [[int(rng.choice([0, 0, 1, 1, 2, 3, 5, 9, 40])) for _ in range(S)] for _ in range(n)]
    quant[3] = [0] * S                                   # no count at all
    if S >= 2:
        quant[5] = [1] * S                               # each sample below a cutoff of 2, the sum at or above it
        quant[7] = [4, 1] + [0] * (S - 2)                # the sum reaches 5, no sample does
    return seqs, quant


def cases():
    out = []
    for S in (1, 2, 3):
        samples = ["s%d.fastq" % k for k in range(S)]
        for spike in (False, True):
            for k, (lo, hi, cc) in enumerate(((16, 25, 2), (16, 25, 1), (16, 25, 5), (20, 20, 2))):
                seqs, quant = world(100 * S + 10 * spike + k, S)
                out.append(dict(name="S%d_spike%d_%d_%d_%d" % (S, spike, lo, hi, cc), samples=samples, spike=spike, min_len=lo,
                                max_len=hi, cutoff=cc, seqs=seqs, quant=quant))
    seqs, quant = world(7, 2)
    out.append(dict(name="one_stem", samples=["a.fastq", "a.trimmed.fastq"], spike=False, min_len=16, max_len=25, cutoff=2,
                    seqs=seqs, quant=quant))
    seqs, quant = world(8, 3)
    out.append(dict(name="one_stem_of_three", samples=["x.1.fastq", "y.fastq", "x.2.fastq"], spike=True, min_len=16, max_len=25,
                    cutoff=2, seqs=seqs, quant=quant))
    out.append(dict(name="empty", samples=["s0.fastq", "s1.fastq"], spike=False, min_len=16, max_len=25, cutoff=2, seqs=[],
                    quant=[]))
    return out


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    tmp, reference = load_reference(sys.argv[1])
    got = []
    try:
        for c in cases():
            work = os.path.join(tmp, c["name"])
            os.makedirs(work)
            text = csv_text(c["samples"], c["seqs"], c["quant"], c["spike"])
            path = os.path.join(work, "unmapped.csv")
            with open(path, "w") as fh:
                fh.write(text)
            out_dir = os.path.join(work, "out")
            os.makedirs(out_dir)
            reference(path, str(c["min_len"]), str(c["max_len"]), str(c["cutoff"]), out_dir, "human", {"human": "hsa"}, c["spike"])
            files = {}
            for fn in sorted(os.listdir(out_dir)):
                with open(os.path.join(out_dir, fn)) as fh:
                    files[fn] = fh.read()
            got.append(dict(name=c["name"], spike=c["spike"], min_len=c["min_len"], max_len=c["max_len"], cutoff=c["cutoff"],
                            csv=text, files=files))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    with open(OUT, "w") as fh:
        json.dump(dict(source="reference utils/convert2Fasta.py", cases=got), fh, indent=0)
    print("wrote %s: %d cases, %d bytes" % (OUT, len(got), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
