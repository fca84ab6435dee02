"""Predict mode's location clusters on the CPU: the sequential model (tests/predict_cluster_model.py) reproduces every
table the reference's own cluster_basedon_location wrote (tests/golden/predict_clusters.json), and the host writers
(mrg_write_clusters, mrg_write_sorted_sam) print hand-made cluster arrays exactly as the model prints them, with one
worker thread and with eight."""
import json
import os

import numpy as np
import pytest

from tests import predict_cluster_model as model
from tests.conftest import ROOT

GOLDEN = os.path.join(ROOT, "tests", "golden", "predict_clusters.json")


def golden_cases():
    with open(GOLDEN) as fh:
        return json.load(fh)["cases"]


def test_model_reproduces_the_reference_tables():
    cases = golden_cases()
    assert len(cases) >= 12
    n = rows = 0
    for c in cases:
        assert sorted(c["tsv"]) == ["1", "14", "15", "8"]
        for t, want in c["tsv"].items():
            assert model.cluster_tsv(c["sam"], int(t), model.sample_of(c["file"])) == want, (c["file"], t)
            n += 1
            rows += want.count("\n") - 1
    assert n >= 48 and rows > 500
    empty = [c for c in cases if not c["sam"]]
    assert empty and all(v == model.HEADER for v in empty[0]["tsv"].values())


def test_golden_inputs_cover_the_stated_shapes():
    cases = golden_cases()
    lines = [l.split("\t") for c in cases for l in c["sam"].splitlines() if l and l[0] != "@"]
    assert {l[1] for l in lines} == {"0", "16", "4"}
    assert any("chr" not in l[2] and l[1] != "4" for l in lines)
    assert any(len(l[9]) > 25 for l in lines) and any("N" in l[9] for l in lines)
    # a threshold matters: some input clusters differently at 14 and at 15
    assert any(c["tsv"]["14"].count("\n") != c["tsv"]["15"].count("\n") for c in cases)
    assert any(c["tsv"]["1"].count("\n") != c["tsv"]["8"].count("\n") for c in cases)


def revcomp(s):
    return s[::-1].translate(str.maketrans("ACGTN", "TGCAN"))


def hand_made_world(n_reads, seed=11):
    """Three entries (one without "chr"), reads cut from them on either strand without mismatches, some unaligned and
    one suppressed: (entry names, entry seqs, read names, read seqs, rows (read, entry, offset, strand), suppressed)."""
    rng = np.random.default_rng(seed)
    names = ["chr1", "contig_9", "chr2"]
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    seqs = [bytearray(acgt[rng.integers(0, 4, 1000000)].tobytes()) for _ in names]
    rnames, rseqs, rows = [], [], []
    supp = np.zeros(n_reads, bool)
    for r in range(n_reads):
        L = int(rng.integers(16, 41))
        rnames.append("mir%d_%d" % (r, int(rng.integers(1, 500))))
        if r % 50 == 7:
            rseqs.append("".join("ACGT"[c] for c in rng.integers(0, 4, L)))
            supp[r] = r % 100 == 7
            continue
        e = int(rng.integers(0, 3))
        at = int(rng.integers(0, len(seqs[e]) - L))
        strand = int(rng.integers(0, 2))
        cut = seqs[e][at:at + L].decode()
        rseqs.append(revcomp(cut) if strand else cut)
        rows.append((r, e, at, strand))
        if r % 9 == 0:   # a second alignment of the same read elsewhere (same bases pasted into the genome)
            e2, at2 = (e + 1) % 3, int(rng.integers(0, 900000))
            seqs[e2][at2:at2 + L] = cut.encode()
            rows.append((r, e2, at2, strand))
    seqs = [s.decode() for s in seqs]
    return names, seqs, rnames, rseqs, rows, supp


def unsorted_sam(names, seqs, rnames, rseqs, rows, supp, m):
    by_read = {}
    for r, e, at, strand in rows:
        by_read.setdefault(r, []).append((e, at, strand))
    out = ["@HD\tVN:1.0\tSO:unsorted\n"] + ["@SQ\tSN:%s\tLN:%d\n" % (n, len(s)) for n, s in zip(names, seqs)]
    for r, (name, q) in enumerate(zip(rnames, rseqs)):
        if r not in by_read:
            out.append("%s\t4\t*\t0\t0\t*\t*\t0\t0\t%s\t%s\tXM:i:%d\n" % (name, q, "I" * len(q), m + 1 if supp[r] else 0))
            continue
        for e, at, strand in by_read[r]:
            s = revcomp(q) if strand else q
            ref = seqs[e][at:at + len(q)]
            md, run = "", 0
            for x, y in zip(s, ref):
                if x == y:
                    run += 1
                else:
                    md += "%d%s" % (run, y)
                    run = 0
            mm = sum(x != y for x, y in zip(s, ref))
            out.append("%s\t%d\t%s\t%d\t255\t%dM\t*\t0\t0\t%s\t%s\tXA:i:%d\tMD:Z:%s%d\tNM:i:%d\n"
                       % (name, 16 if strand else 0, names[e], at + 1, len(q), s, "I" * len(q), mm, md, run, mm))
    return "".join(out)


def arrays_from_tsv(tsv, entry_names, rnames):
    """The model's table back as the cluster arrays of Engine.cluster_valid."""
    index = {n: i for i, n in enumerate(rnames)}
    entry, strand, start, end, seq, csum, moff, members = [], [], [], [], [], [], [0], []
    for line in tsv.splitlines()[1:]:
        f = line.split("\t")
        entry.append(entry_names.index(f[1]))
        strand.append(f[2] == "-")
        start.append(int(f[3]))
        end.append(int(f[4]))
        seq.append(f[5])
        csum.append(int(f[7]))
        members += [index[x] for x in f[9].split(",")]
        moff.append(len(members))
    soff = np.zeros(len(seq) + 1, dtype=np.uint64)
    np.cumsum([len(s) for s in seq], out=soff[1:])
    return dict(entry=np.array(entry, np.uint32), strand=np.array(strand, np.uint8), start=np.array(start, np.uint32),
                end=np.array(end, np.uint32), seq_off=soff, seq="".join(seq).encode(), count_sum=np.array(csum, np.uint64),
                member_off=np.array(moff, np.uint32), members=np.array(members, np.uint32))


@pytest.mark.parametrize("threshold", [1, 14])
def test_writers_match_the_model_for_1_and_8_threads(native_lib, tmp_path, threshold):
    from mirge_amd import predict
    from mirge_amd.index import FmIndex
    names, seqs, rnames, rseqs, rows, supp = hand_made_world(72000)
    m = 3
    text = unsorted_sam(names, seqs, rnames, rseqs, rows, supp, m)
    want_sam = model.sort_sam(text)
    sam_name = "unmapped_mirna_S1_vs_genome_sorted.sam"
    want_tsv = model.cluster_tsv(want_sam, threshold, model.sample_of(sam_name))
    assert want_tsv.count("\n") > 8192 + 1          # more clusters than one formatting block
    assert predict.sample_name(str(tmp_path / sam_name)) == "unmapped_mirna_S1"
    cl = arrays_from_tsv(want_tsv, names, rnames)
    ix = [FmIndex.build(names[:2], seqs[:2]), FmIndex.build(names[2:], seqs[2:])]   # two parts, entries numbered on
    order = sorted(range(len(rows)), key=lambda k: (rows[k][1], rows[k][2], rows[k][3], k))
    mm = [sum(x != y for x, y in zip(revcomp(rseqs[r]) if st else rseqs[r], seqs[e][at:at + len(rseqs[r])]))
          for r, e, at, st in rows]       # (a later paste may have changed bases under an earlier read)
    cols = tuple(np.array([rows[k][c] for k in order]) for c in range(4)) + (np.array([mm[k] for k in order], np.uint8),)
    assert len(rows) > 65536
    for threads in (1, 8):
        tsv = tmp_path / ("t%d.tsv" % threads)
        assert predict.write_clusters(str(tsv), "unmapped_mirna_S1", ix, rnames, cl, threads=threads) == len(cl["entry"])
        assert tsv.read_text() == want_tsv
        sam = tmp_path / ("t%d.sam" % threads)
        s = predict.write_sorted_sam(str(sam), ix, rnames, rseqs, cols, supp, m, threads=threads)
        assert sam.read_text() == want_sam
        assert s["reported"] == len(rows) and s["suppressed"] == int(supp.sum())
        assert s["aligned"] == len({r[0] for r in rows})
    assert "MIRGE_AMD_TABLE_THREADS" not in os.environ


def test_empty_cluster_table_is_the_header_line(native_lib, tmp_path):
    from mirge_amd import predict
    from mirge_amd.index import FmIndex
    ix = [FmIndex.build(["chr1"], ["ACGTACGTACGTACGTACGTAGCTAGCTAGCATCGATCGAT"])]
    cl = arrays_from_tsv(model.HEADER, ["chr1"], [])
    p = tmp_path / "e.tsv"
    assert predict.write_clusters(str(p), "s", ix, ["mir0_4"], cl) == 0
    assert p.read_text() == model.HEADER == predict.HEADER
    q = tmp_path / "e.sam"
    none = tuple(np.zeros(0, dt) for dt in (np.uint32, np.int32, np.int32, np.uint8, np.uint8))
    predict.write_sorted_sam(str(q), ix, ["mir0_4"], ["ACGTTGCATTGACC"], none, np.zeros(1, bool), 3)
    assert q.read_text() == "@HD\tVN:1.0\tSO:coordinate\n@SQ\tSN:chr1\tLN:41\n" \
                            "mir0_4\t4\t*\t0\t0\t*\t*\t0\t0\tACGTTGCATTGACC\tIIIIIIIIIIIIII\tXM:i:0\n"


def test_read_counts_come_from_the_names(native_lib):
    from mirge_amd import predict
    assert predict.read_counts(["mir1_5", "mir22_4000000000", "mir3_17_extra"]).tolist() == [5, 4000000000, 17]
    assert predict.read_counts([]).tolist() == []
    for bad in ("mir5", "mir5_", "mir5_x2", "mir_5000000000"):
        with pytest.raises(ValueError):
            predict.read_counts(["mir1_1", bad])
