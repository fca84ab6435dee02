"""Predict mode's map-and-cluster call on the GPU (-m gpu): mirge_amd.predict.map_and_cluster writes, for the small
libraries and the three-part genome world of tests/test_gpu_bowtie.py, exactly the cluster table that the sequential
model (tests/predict_cluster_model.py) makes of the text model's SAM (tests/bowtie_text_model.py) sorted by coordinate,
and a sorted SAM file equal to it in row order and in the columns the reference reads; and at 10^6 rows the cluster
arrays keep the rule's invariants and do not depend on how the genome is split into parts."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import bowtie_text_model as btm
from tests import predict_cluster_model as model
from tests.conftest import ROOT
from tests.test_bowtie_cli import random_world
from tests.test_gpu_bowtie import genome_world, write_parts

pytestmark = pytest.mark.gpu


def as_collapsed(fasta):
    """The reads renamed as the reference's collapsed reads: mir<k>_<count>."""
    k = [0]

    def name(_):
        k[0] += 1
        return ">mir%d_%d" % (k[0], 1 + (k[0] * 13) % 41)
    return re.sub(r"^>\S+", name, fasta, flags=re.M)


def expected(parts, fasta, mapping_loc, sam_name):
    """(sorted SAM text, {threshold: TSV text}) from the two models."""
    argv = ["-f", "-n", "0"] + (["-m", str(mapping_loc)] if mapping_loc else []) + ["-l", "25", "-S", "-a", "--best", "g", "r.fa"]
    out, _ = btm.run(argv, parts, fasta)
    sam = model.sort_sam(out)
    return sam, {t: model.cluster_tsv(sam, t, model.sample_of(sam_name)) for t in (1, 14, 15)}


def columns(sam_text):
    """Header lines whole; of the other lines the columns the reference reads (1-4 and 10)."""
    rows = []
    for line in sam_text.splitlines():
        f = line.split("\t")
        rows.append(line if line[0] == "@" else (f[0], f[1], f[2], f[3], f[9]))
    return rows


def overlap_reads(parts):
    """Four more reads from a stretch of the first entry that occurs once in the genome: two that overlap by 14 bases
    (one cluster at thresholds 1 and 14, two at 15) and two that overlap by 5 (one cluster at threshold 1 only), so that
    every threshold of the tests changes the table whatever -m suppresses."""
    seqs = [s for _, ss in parts for s in ss]
    comp = str.maketrans("ACGTN", "TGCAN")
    src = seqs[0]
    for a in range(1000, len(src) - 100, 97):
        cuts = [src[a:a + 20], src[a + 6:a + 26], src[a + 40:a + 60], src[a + 55:a + 75]]
        if "N" in src[a:a + 75]:
            continue
        if all(sum(s.count(q) + s.count(q[::-1].translate(comp)) for s in seqs) == 1 for q in cuts):
            return "".join(">extra%d\n%s\n" % (i, q) for i, q in enumerate(cuts))
    raise AssertionError("no unique stretch in the first entry")


@pytest.fixture(scope="module")
def engine(native_lib):
    from mirge_amd.engine import Engine
    eng = Engine(0)
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def genome(tmp_path_factory, native_lib, oracle_lib):
    d = tmp_path_factory.mktemp("predict_genome")
    parts, fasta = genome_world(77)
    fasta = as_collapsed(fasta + overlap_reads(parts))
    write_parts(parts, str(d / "g"))
    (d / "reads.fa").write_text(fasta)
    return d, parts, fasta


@pytest.mark.parametrize("mapping_loc", [1, 3, 0])
def test_genome_parts_equal_the_models(genome, engine, tmp_path, mapping_loc):
    from mirge_amd import predict
    d, parts, fasta = genome
    stem = str(tmp_path / "unmapped_mirna_S7")
    want_sam, want_tsv = expected(parts, fasta, mapping_loc, stem + "_vs_genome_sorted.sam")
    assert want_tsv[14].count("\n") > 50
    assert any("\t-\t" in l for l in want_tsv[14].splitlines()) and any("\t+\t" in l for l in want_tsv[14].splitlines())
    for t in (1, 14, 15):
        cl = predict.map_and_cluster(engine, str(d / "reads.fa"), str(d / "g"), mapping_loc, 25, t, stem)
        assert open(stem + "_vs_genome_sorted_clusters.tsv").read() == want_tsv[t], (mapping_loc, t)
        assert columns(open(stem + "_vs_genome_sorted.sam").read()) == columns(want_sam)
        assert len(cl["entry"]) == want_tsv[t].count("\n") - 1
    if mapping_loc:
        assert cl["suppressed"].any()        # (the 10^4- and 40-copy reads)
    assert want_tsv[1] != want_tsv[14] and want_tsv[14] != want_tsv[15]      # (overlap_reads)


def test_entries_without_chr_are_left_out_and_no_sam_is_optional(engine, tmp_path, native_lib, oracle_lib):
    """The small libraries' entries are named p<k>e<j>: their alignments fill the sorted SAM and no cluster; with one
    part renamed, that part's clusters appear and are numbered from 1."""
    from mirge_amd import predict
    parts, fasta = random_world(2024, n_parts=2, entries=6, n_reads=600)
    fasta = as_collapsed(fasta)
    (tmp_path / "reads.fa").write_text(fasta)
    for k, renamed in enumerate((parts, [parts[0], (["chr_" + n for n in parts[1][0]], parts[1][1])])):
        prefix = str(tmp_path / ("lib%d" % k))
        write_parts(renamed, prefix)
        stem = str(tmp_path / ("mapped_mirna_x%d" % k))
        want_sam, want_tsv = expected(renamed, fasta, 3, stem + "_vs_genome_sorted.sam")
        predict.map_and_cluster(engine, str(tmp_path / "reads.fa"), prefix, 3, 25, 14, stem)
        got = open(stem + "_vs_genome_sorted_clusters.tsv").read()
        assert got == want_tsv[14]
        assert (got == model.HEADER) == (k == 0)
        assert columns(open(stem + "_vs_genome_sorted.sam").read()) == columns(want_sam)
    os.remove(stem + "_vs_genome_sorted.sam")
    predict.map_and_cluster(engine, str(tmp_path / "reads.fa"), prefix, 3, 25, 14, stem, sam=False)
    assert not os.path.exists(stem + "_vs_genome_sorted.sam")
    assert open(stem + "_vs_genome_sorted_clusters.tsv").read() == want_tsv[14]


def test_no_alignment_and_no_read_give_the_header_line(genome, engine, tmp_path):
    from mirge_amd import predict
    d, parts, _ = genome
    rng = np.random.default_rng(5)
    reads = tmp_path / "none.fa"
    reads.write_text("".join(">mir%d_3\n%s\n" % (i, "".join("ACGT"[c] for c in rng.integers(0, 4, 24))) for i in range(40)))
    stem = str(tmp_path / "mapped_mirna_none")
    cl = predict.map_and_cluster(engine, str(reads), str(d / "g"), 3, 25, 14, stem)
    assert cl["n_rows"] == 0 and open(stem + "_vs_genome_sorted_clusters.tsv").read() == model.HEADER
    sam = open(stem + "_vs_genome_sorted.sam").read().splitlines()
    assert sam[0] == "@HD\tVN:1.0\tSO:coordinate" and sum(l.split("\t")[1] == "4" for l in sam if l[0] != "@") == 40
    reads.write_text("")
    predict.map_and_cluster(engine, str(reads), str(d / "g"), 3, 25, 14, stem)
    assert open(stem + "_vs_genome_sorted_clusters.tsv").read() == model.HEADER


def test_limits_and_bad_names_are_errors_that_write_nothing(genome, engine, tmp_path):
    from mirge_amd import predict
    d, _, _ = genome
    stem = str(tmp_path / "mapped_mirna_bad")
    reads = tmp_path / "bad.fa"
    reads.write_text(">mir1_2\n" + "ACGT" * 64 + "\n")
    with pytest.raises(ValueError, match="255"):
        predict.map_and_cluster(engine, str(reads), str(d / "g"), 3, 25, 14, stem)
    reads.write_text(">g1\nACGTACGTACGTACGTACGT\n")
    with pytest.raises(ValueError, match="count"):
        predict.map_and_cluster(engine, str(reads), str(d / "g"), 3, 25, 14, stem)
    reads.write_text(">mir1_2\nACGTACGTACGTACGTACGT\n")
    with pytest.raises(ValueError, match="overlapLenCutoff"):
        predict.map_and_cluster(engine, str(reads), str(d / "g"), 3, 25, 0, stem)
    assert not [f for f in os.listdir(str(tmp_path)) if f.startswith("mapped_mirna_bad")]


def test_command_line_writes_both_files(genome, tmp_path):
    d, parts, fasta = genome
    stem = str(tmp_path / "unmapped_mirna_cli")
    r = subprocess.run([sys.executable, "-m", "mirge_amd.predict", "clusters", str(d / "g"), str(d / "reads.fa"), "-m", "3", "-l",
                        "25", "--overlap", "14", "-o", stem], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    want_sam, want_tsv = expected(parts, fasta, 3, stem + "_vs_genome_sorted.sam")
    assert open(stem + "_vs_genome_sorted_clusters.tsv").read() == want_tsv[14]
    assert columns(open(stem + "_vs_genome_sorted.sam").read()) == columns(want_sam)


# ---------------------------------------------------------------------------------------------------------- 10^6 rows
def big_world(seed=31, n_entries=6, entry_bases=1500000, n_reads=1000000):
    """Entries (one without "chr") and distinct reads of 16-25 nt (a few of 30) cut from them on either strand, drawn in piles around
    loci so that clusters of every size form; a few reads with an N."""
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    names = ["chr%d" % (i + 1) for i in range(n_entries)]
    names[2] = "scaffold_3"
    texts = [acgt[rng.integers(0, 4, entry_bases)].tobytes() for _ in names]
    loci = rng.integers(100, entry_bases - 100, 60000)
    loci_e = rng.integers(0, n_entries, loci.size)
    pick = rng.integers(0, loci.size, n_reads * 2)
    at = loci[pick] + rng.integers(-30, 31, pick.size)
    L = rng.integers(16, 26, pick.size)
    strand = rng.integers(0, 2, pick.size)
    comp = bytes.maketrans(b"ACGT", b"TGCA")
    seen, lines = set(), []
    for e, a, l, s in zip(loci_e[pick].tolist(), at.tolist(), L.tolist(), strand.tolist()):
        with_n = len(lines) % 5000 == 17      # 30 nt with an N past the 25-nt seed: it aligns, and its N is printed
        q = texts[e][a:a + (30 if with_n else l)]
        if q in seen:
            continue
        seen.add(q)
        if s:
            q = q[::-1].translate(comp)
        if with_n:
            q = q[:27] + b"N" + q[28:]
        lines.append(b">mir%d_%d\n%s\n" % (len(lines), 1 + len(lines) % 97, q))
        if len(lines) == n_reads:
            break
    return names, [t.decode() for t in texts], b"".join(lines)


def test_million_rows_keep_the_invariants_and_ignore_the_split(engine, tmp_path, native_lib):
    from mirge_amd import bowtie, pack, predict
    from mirge_amd.engine import ReadSet, STRATUM_ALL
    from mirge_amd.index import FmIndex
    names, texts, fasta = big_world()
    (tmp_path / "reads.fa").write_bytes(fasta)
    FmIndex.build(names, texts).save(str(tmp_path / "one.mrgfm"))
    for k in range(3):
        FmIndex.build(names[2 * k:2 * k + 2], texts[2 * k:2 * k + 2]).save("%s.part%03d.mrgfm" % (tmp_path / "three", k))
    t = 14
    files = []
    for prefix in ("one", "three"):
        os.mkdir(str(tmp_path / ("out_" + prefix)))      # (the same file name both times: the sample name is printed)
        stem = str(tmp_path / ("out_" + prefix) / "mapped_mirna_big")
        cl = predict.map_and_cluster(engine, str(tmp_path / "reads.fa"), str(tmp_path / prefix), 3, 25, t, stem)
        files.append((open(stem + "_vs_genome_sorted_clusters.tsv", "rb").read(), open(stem + "_vs_genome_sorted.sam", "rb").read()))
    assert files[0][0] == files[1][0], "the cluster table depends on the split into parts"
    assert files[0][1] == files[1][1], "the sorted SAM depends on the split into parts"
    print("rows %d, on chr entries %d, clusters %d" % (cl["n_rows"], cl["n_valid"], len(cl["entry"])))
    assert cl["n_rows"] > 900000
    entry, strand, start, end = (cl[k].astype(np.int64) for k in ("entry", "strand", "start", "end"))
    C = len(entry)
    assert C > 10000
    # clusters are ordered by list, and inside a list every cluster starts past the previous one's end - t + 1
    lst = entry * 2 + strand
    assert (np.diff(lst) >= 0).all()
    same = lst[1:] == lst[:-1]
    assert same.any() and (start[1:][same] > end[:-1][same] - t + 1).all()
    assert (start[1:][same] >= start[:-1][same]).all()
    # members: every reportable row on a chr entry, once
    names_r, seqs = bowtie.read_fasta(str(tmp_path / "reads.fa"))
    words, lens, nmask = pack.pack_reads(seqs, 1)
    keys, parts = predict.genome_libraries(engine, str(tmp_path / "three"))
    off, l_entry, l_off, l_strand, l_mm, supp = engine.list_valid(ReadSet(words, lens, nmask, device=engine.device), keys,
                                                                 strands=2, stratum_mode=STRATUM_ALL, m=3, seed_len=25,
                                                                 max_mm_seed=0, max_mm_total=2)
    keep = np.array(["chr" in n for n in names])
    on_chr = keep[l_entry]
    assert cl["n_rows"] == len(l_entry) and (~on_chr).any()
    member_off = cl["member_off"].astype(np.int64)
    n_members = np.diff(member_off)
    assert n_members.min() >= 1 and n_members.max() > 3
    assert int(n_members.sum()) == int(on_chr.sum()) == cl["n_valid"] == len(cl["members"])
    assert keep[entry].all()
    owner = np.repeat(np.arange(len(seqs)), np.diff(off))
    assert np.array_equal(np.sort(cl["members"].astype(np.int64)), np.sort(owner[on_chr]))
    assert np.array_equal(supp, cl["suppressed"])
    # read-count sums
    counts = predict.read_counts(names_r).astype(np.uint64)
    assert np.array_equal(np.add.reduceat(counts[cl["members"]], member_off[:-1]), cl["count_sum"])
    # sequences: one base per position, the head's read first
    seq_len = np.diff(cl["seq_off"].astype(np.int64))
    assert np.array_equal(seq_len, end - start + 1) and int(cl["seq_off"][-1]) == len(cl["seq"])
    assert set(cl["seq"]) <= set(b"ACGTN") and b"N" in cl["seq"]
    comp = str.maketrans("ACGTN", "TGCAN")
    for c in np.random.default_rng(1).integers(0, C, 2000).tolist():
        q = seqs[int(cl["members"][member_off[c]])]
        if strand[c]:
            q = q[::-1].translate(comp)
        assert cl["seq"][int(cl["seq_off"][c]):int(cl["seq_off"][c]) + len(q)].decode() == q
