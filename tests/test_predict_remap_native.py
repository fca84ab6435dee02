"""Predict mode's second mapping without a GPU: the model (tests/predict_remap_model.py) against the golden tables of the
reference's processSam functions and `LC_ALL=C sort -k6,6 -k1,1` (tests/golden/predict_remap.json), the native writer
(mrg_write_remapped_rows) fed the model's rows, its block order on four threads, the argument checks, the options and the
key rule."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from tests import bowtie_text_model as btm
from tests import predict_remap_model as model

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "predict_remap.json")
with open(GOLDEN) as fh:
    WORLDS = json.load(fh)["worlds"]


def model_route(w):
    """bowtie_text_model twice, then the model: (table text, sorted rows)."""
    parts = [model.parse_fasta(w["clusters_fa"])]
    sam1, _ = btm.run(model.pass1_argv(w["seed_length"]) + ["ix", "reads.fa"], parts, w["reads_fa"])
    sam2, _ = btm.run(model.PASS2_ARGV + ["ix", "left.fa"], parts, model.unaligned_fasta(sam1, w["reads_fa"]))
    return model.table_from_sam(sam1, sam2, w["reads_fa"], w["clusters_fa"])


def write_rows(tmp_path, clusters_fa, names, seqs, rows, threads=None, out="out.tsv"):
    """mrg_write_remapped_rows over the model's rows; the cluster library is built on the host from the FASTA text."""
    from mirge_amd import pack, predict
    from mirge_amd.index import FmIndex
    fa = tmp_path / "clusters_orig.fa"
    fa.write_text(clusters_fa)
    _, _, _, soff, orig = model.cluster_arrays(clusters_fa)
    index = FmIndex.from_fasta(str(fa))
    words, lens, nmask = pack.pack_reads(seqs) if seqs else (np.zeros((1, 0), np.uint64), np.zeros(0, np.uint8), None)
    numbers = [model.read_number(n) for n in names]
    counts = [int(n.split("_")[-1]) for n in names]
    cols = tuple(np.array([r[k] for r in rows], dtype=np.uint32 if k < 3 else np.uint8) for k in range(5))
    path = str(tmp_path / out)
    n = predict.write_remapped_rows(path, words, lens, nmask, numbers, counts, index, soff, orig, cols, threads=threads)
    assert n == len(rows)
    return open(path).read()


@pytest.mark.parametrize("w", WORLDS, ids=lambda w: w["name"])
def test_model_reproduces_the_golden_tables(oracle_lib, w):
    text, rows = model_route(w)
    assert text == w["table"]
    assert len(rows) == w["table"].count("\n")


def test_golden_worlds_hold_every_case():
    held = set(h for w in WORLDS for h in w["holds"])
    assert {"seed_length_25", "seed_length_18", "one_cluster_exact", "several_clusters", "no_alignment", "pass2_first_base",
            "pass2_three_prime", "pass2_seed_mismatch_row", "better_stratum_competitor", "two_offsets_one_cluster",
            "cluster_numbers_cross", "read_numbers_cross", "n_in_read", "empty_result"} <= held
    assert all(len(model.parse_fasta(w["reads_fa"])[0]) <= 100 for w in WORLDS)


@pytest.mark.parametrize("w", WORLDS, ids=lambda w: w["name"])
def test_native_writer_on_the_models_rows(native_lib, oracle_lib, tmp_path, w):
    _, rows = model_route(w)
    names, seqs = model.parse_fasta(w["reads_fa"])
    assert write_rows(tmp_path, w["clusters_fa"], names, seqs, rows) == w["table"]
    # the rows of one read on one cluster in the other order: the writer settles them
    flipped, k = [], 0
    while k < len(rows):
        e = k + 1
        while e < len(rows) and rows[e][:2] == rows[k][:2]:
            e += 1
        flipped += rows[k:e][::-1]
        k = e
    assert write_rows(tmp_path, w["clusters_fa"], names, seqs, flipped, out="flipped.tsv") == w["table"]


def big_world():
    rng = np.random.default_rng(71)
    rnd = lambda n: "".join("ACGT"[c] for c in rng.integers(0, 4, n))
    numbers = sorted(int(x) for x in rng.choice(np.arange(1, 1200), 50, replace=False))
    cseqs = [rnd(40) for _ in numbers]
    clusters_fa = "".join(">smp:miRCluster_%d_40:chr1:%d_%d+\n%s\n" % (i, 10 * i, 10 * i + 39, s) for i, s in zip(numbers, cseqs))
    rn = sorted(int(x) for x in rng.choice(np.arange(1, 3000), 380, replace=False))
    names = ["mir%d_%d" % (n, int(rng.integers(2, 99))) for n in rn]
    seqs = [rnd(int(rng.integers(16, 26))) for _ in names]
    seqs[5] = seqs[5][:7] + "N" + seqs[5][8:]
    rows = []
    for r in range(len(names)):
        for c in range(len(cseqs)):
            second = (r + c) % 3 == 0
            rows.append((r, c, int(rng.integers(0, 5)), int(rng.integers(0, 3)), int(second)))
            if (r * 7 + c) % 19 == 0:                     # the same read twice, sometimes three times, on one cluster
                rows.append((r, c, int(rng.integers(5, 9)), 0, int(second)))
                if c % 2:
                    rows.append((r, c, 9 + c % 2, 1, int(second)))
    rows = [rows[int(j)] for j in rng.permutation(len(rows))]
    return clusters_fa, numbers, cseqs, names, seqs, rows


def test_20000_rows_on_four_threads_stay_in_order(native_lib, tmp_path, monkeypatch):
    clusters_fa, numbers, cseqs, names, seqs, rows = big_world()
    assert len(rows) >= 20000
    cnames = model.parse_fasta(clusters_fa)[0]
    srt = model.sort_rows(rows, [model.read_number(n) for n in names], numbers)
    want = model.table(srt, names, seqs, cnames, cseqs)
    assert write_rows(tmp_path, clusters_fa, names, seqs, srt, threads=4) == want
    assert write_rows(tmp_path, clusters_fa, names, seqs, srt, threads=1, out="one.tsv") == want
    monkeypatch.setenv("MIRGE_AMD_PREDICT_BLOCK_ROWS", "7")     # blocks that end inside the runs of one read on one cluster
    assert write_rows(tmp_path, clusters_fa, names, seqs, srt, threads=4, out="small.tsv") == want


def test_key_rule_agrees_with_sorted_on_the_name_strings():
    rng = np.random.default_rng(9)
    pick = lambda: int(rng.choice([rng.integers(1, 12), rng.integers(1, 120), rng.integers(90, 1100), rng.integers(1, 2 ** 32)]))
    lens = {}
    pairs = []
    for _ in range(10000):
        i, n = pick(), pick()
        lens.setdefault(i, int(rng.integers(16, 31)))
        pairs.append((i, n))
    cname = lambda i: ("smp:miRCluster_%d_%d:chr1:5_%d+" % (i, lens[i], 4 + lens[i])).encode()
    rname = lambda n: ("mir%d_%d" % (n, n % 7 + 2)).encode()
    by_name = sorted(pairs, key=lambda p: (cname(p[0]), rname(p[1])))
    by_key = sorted(pairs, key=lambda p: (model.name_key(p[0]), model.name_key(p[1])))
    assert by_name == by_key
    assert model.name_key(10) < model.name_key(1) < model.name_key(2) and model.name_key(2 ** 32 - 1) < 2 ** 40


def test_writer_refuses_contradictory_arguments_before_opening_the_file(native_lib, tmp_path):
    from mirge_amd._native import MirgeAmdError
    w = WORLDS[0]
    names, seqs = model.parse_fasta(w["reads_fa"])
    cnames, cseqs = model.parse_fasta(w["clusters_fa"])
    good = (0, 0, 0, 0, 0)
    assert len(seqs[0]) <= len(cseqs[0])                       # (the good row fits its cluster)
    for bad, what in (((len(names), 0, 0, 0, 0), b"unknown read"), ((0, len(cnames), 0, 0, 0), b"unknown cluster"),
                      ((0, 0, 0, 0, 2), b"unknown pass"), ((0, 0, len(cseqs[0]), 0, 0), b"past the end")):
        with pytest.raises(MirgeAmdError):
            write_rows(tmp_path, w["clusters_fa"], names, seqs, [good, bad], out="never.tsv")
        assert what in native_lib.mrg_last_error()
        assert not os.path.exists(str(tmp_path / "never.tsv"))
    with pytest.raises(MirgeAmdError):                          # a read of four bases has nothing left in pass 2
        write_rows(tmp_path, w["clusters_fa"], ["mir1_2"], ["ACGT"], [(0, 0, 0, 0, 1)], out="never.tsv")
    assert b"empty read" in native_lib.mrg_last_error() and not os.path.exists(str(tmp_path / "never.tsv"))
    with pytest.raises(ValueError):                             # a library of another size than the cluster arrays
        from mirge_amd import predict
        from mirge_amd.index import FmIndex
        predict.write_remapped_rows(str(tmp_path / "never.tsv"), np.zeros((1, 1), np.uint64), [4], None, [1], [2],
                                    FmIndex.build(["a"], ["ACGTACGTACGTACGTAC"]), [0, 5, 9], b"ACGTAACGT",
                                    tuple(np.zeros(0, np.uint32) for _ in range(5)))
    L = native_lib
    out = C.c_uint64()
    assert L.mrg_write_remapped_rows(None, None, 1, 0, None, None, 0, None, None, None, 0, None, None, 0, None, None, None, None, None,
                                     1, 3, C.byref(out)) < 0 and b"null" in L.mrg_last_error()
    assert L.mrg_write_remapped_rows(b"x", None, 1, 0, None, None, 0, None, None, None, 0, None, None, 3, None, None, None, None, None,
                                     1, 3, C.byref(out)) < 0 and b"null row arrays" in L.mrg_last_error()
    assert L.mrg_predict_remap_temp_bytes(10, 10, None) < 0 and b"null" in L.mrg_last_error()
    assert L.mrg_predict_remap_temp_bytes(2 ** 31, 10, C.byref(out)) < 0 and b"reads" in L.mrg_last_error()
    assert L.mrg_predict_remap_temp_bytes(10, 2 ** 32 - 1, C.byref(out)) < 0 and b"rows" in L.mrg_last_error()
    assert L.mrg_predict_remap_temp_bytes(1000, 5000, C.byref(out)) == 0 and out.value >= 5000 * 46
    assert L.mrg_predict_trim_reads(None, None, 1, 0, None, None, 0, None, 1, 3, None, None, None, None, C.byref(out), None, 0, None) < 0
    assert L.mrg_predict_remap_rows(None, 0, None, 0, None, None, 0, None, None, None, 0, None, None, 0, None, None, None, None, None,
                                    None, None, None, None, 0, None) < 0 and b"null" in L.mrg_last_error()


def test_options_are_off_by_default_and_novel_map_implies_the_trim():
    import inspect
    from mirge_amd import cli, predict
    ap = cli.build_parser()
    base = ["annotate", "-s", "x.fastq", "-lib", "libs", "-sp", "human"]
    assert cli.novel_stages(ap.parse_args(base)) == (False, False, False, False)
    assert cli.novel_stages(ap.parse_args(base + ["--novel-trim"])) == (True, True, True, False)
    assert cli.novel_stages(ap.parse_args(base + ["--novel-map", "-sl", "18"])) == (True, True, True, True)
    assert ap.parse_args(base + ["--novel-map", "-sl", "18"]).seedLength == "18"
    for fn in (predict.map_and_cluster, predict.map_and_cluster_reads):
        assert inspect.signature(fn).parameters["remap"].default is False
    with pytest.raises(ValueError, match="remap needs trim"):
        predict._map_cluster_write(None, None, None, [], [], "g", 3, 25, 14, "stem", True, None, trim=None, remap=True)
    with pytest.raises(SystemExit):
        predict.main(["clusters", "genome", "reads.fa", "-o", "stem", "--remap"])
    assert predict.REMAP_SUFFIX == "_vs_representative_seq_modified_selected_sorted.tsv" and predict.REMAP_TRIMS == (1, 3)
    assert [model.trim(s) for s in ("", "ACG", "ACGT", "ACGTA", "ACGTACGT")] == ["", "", "", "C", "CGTA"]
