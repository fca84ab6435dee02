"""The host side of predict mode's trim stage without a GPU: mrg_write_trimmed_clusters fed the model's arrays writes the
reference's three files byte for byte (tests/golden/predict_trim.json), predict.load_repeats, the argument checks of the
new entry points and the new command-line options."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from tests import predict_trim_model as model

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "predict_trim.json")
with open(GOLDEN) as fh:
    WORLDS = json.load(fh)["worlds"]
SUFFIXES = ("_trimmed.tsv", "_trimmed.fa", "_trimmed_orig.fa")


def genome(entries):
    from mirge_amd.index import FmIndex
    return [FmIndex.build(list(entries), ["ACGTTGCAAC" * 3] * len(entries))]


def write_world(w, tmp_path, threads=None):
    """The three files of world w by the native writer from the model's flag / rep / orig -> their texts."""
    from mirge_amd import predict
    entries, rows, a, names, count_sum, member_off, members, rep_tsv = model.world_inputs(w["table"], w["elements"])
    rep_file = tmp_path / "repeats.tsv"
    rep_file.write_text(rep_tsv)
    repeats = predict.load_repeats(str(rep_file), genome(entries))
    want = model.flat_repeats(entries, w["elements"])
    assert repeats["rep_off"].tolist() == want[0] and repeats["start"].tolist() == want[1] and repeats["end"].tolist() == want[2]
    assert [repeats["names"][k] for k in repeats["name_id"]] == [want[4][k] for k in want[3]]
    t = model.trim(a["entry"], a["strand"], a["start"], a["end"], a["seq_off"], a["seq"], want[0], want[1], want[2], w["cutoff"])
    cl = dict(a, seq=a["seq"].encode(), count_sum=count_sum, member_off=member_off, members=members)
    stem = str(tmp_path / "out_clusters")
    got = predict.write_trimmed_clusters(stem, "smp", names, cl, dict(flag=t["flag"], rep=t["rep"], orig=t["orig"].encode()),
                                         repeats, threads=threads)
    assert got == (len(rows), sum(t["flag"]))
    return [open(stem + sfx).read() for sfx in SUFFIXES]


@pytest.mark.parametrize("w", WORLDS, ids=lambda w: w["name"])
def test_writer_reproduces_the_golden_files(native_lib, tmp_path, w):
    got = write_world(w, tmp_path)
    if w["ties"]:   # pinned against the model only
        assert got == list(model.files(w["table"], w["elements"], w["cutoff"]))
    else:
        assert got == [w["trimmed_tsv"], w["trimmed_fa"], w["trimmed_orig_fa"]]


def test_empty_table_and_many_blocks_in_order(native_lib, tmp_path):
    w = next(w for w in WORLDS if w["name"] == "empty")
    (tmp_path / "e").mkdir()
    tsv, fa, fo = write_world(w, tmp_path / "e")
    assert tsv.count("\n") == 1 and tsv.startswith("miRClusterID\tOriginalSeq\tFlag\trepetitiveElementName\tChr\tStrand\t")
    assert fa == "" and fo == ""
    # more clusters than one writer block holds, several threads: the rows stay in table order in all three files
    base = next(w for w in WORLDS if w["name"] == "many_elements")
    _, rows = model.parse_table(base["table"])
    lines = []
    for i in range(20000):
        r = list(rows[i % len(rows)])
        r[0] = "smp:miRCluster_%d_%d" % (i + 1, len(r[5]))
        lines.append("\t".join(r) + "\n")
    big = dict(base, table=base["table"].split("\n")[0] + "\n" + "".join(lines))
    (tmp_path / "b").mkdir()
    assert write_world(big, tmp_path / "b", threads=4) == list(model.files(big["table"], big["elements"], big["cutoff"]))


def test_null_and_invalid_arguments(native_lib, tmp_path):
    L = native_lib
    out = C.c_uint64()
    assert L.mrg_predict_trim_temp_bytes(10, None) < 0 and b"null" in L.mrg_last_error()
    assert L.mrg_predict_trim_temp_bytes(2 ** 31, C.byref(out)) < 0 and b"2^31" in L.mrg_last_error()
    assert L.mrg_predict_trim_temp_bytes(4097, C.byref(out)) == 0 and out.value >= 16 + 3 * 4 * 4098 + 8 * 4098
    # a compute entry point does not run without a context (and so without a GPU)
    assert L.mrg_predict_trim(None, 0, None, None, None, None, None, None, 0, 0, None, None, None, 0, 30, None, None, None, None,
                              None, None, C.byref(out), C.byref(out), None, 0, None) < 0
    assert b"mrg_predict_trim: null" in L.mrg_last_error()
    p = [os.fsencode(str(tmp_path / n)) for n in ("a.tsv", "a.fa", "a_orig.fa")]
    rows, kept = C.c_uint64(), C.c_uint64()
    tail = (0, None, None, None, None, None, None, None, None, None, 0, None, None, None, None, None, 0, None, 0, None, None)
    assert L.mrg_write_trimmed_clusters(None, p[1], p[2], b"s", None, 0, *tail, C.byref(rows), C.byref(kept)) < 0
    assert L.mrg_write_trimmed_clusters(p[0], p[1], p[2], None, None, 0, *tail, C.byref(rows), C.byref(kept)) < 0
    assert L.mrg_write_trimmed_clusters(p[0], p[1], p[2], b"s", None, 0, *tail, None, C.byref(kept)) < 0
    assert b"null" in L.mrg_last_error()
    one = (1,) + tail[1:]
    assert L.mrg_write_trimmed_clusters(p[0], p[1], p[2], b"s", None, 0, *one, C.byref(rows), C.byref(kept)) < 0
    assert b"null cluster arrays" in L.mrg_last_error() and not any(os.path.exists(x) for x in p)
    # an element index beyond the table, arrays of the wrong size: refused before a file is opened
    from mirge_amd import predict
    from mirge_amd._native import MirgeAmdError
    w = next(w for w in WORLDS if w["name"] == "two_elements")
    entries, rows_, a, names, count_sum, member_off, members, rep_tsv = model.world_inputs(w["table"], w["elements"])
    (tmp_path / "r.tsv").write_text(rep_tsv)
    repeats = predict.load_repeats(str(tmp_path / "r.tsv"), genome(entries))
    cl = dict(a, seq=a["seq"].encode(), count_sum=count_sum, member_off=member_off, members=members)
    K = len(rows_)
    t = dict(flag=[1] * K, rep=[-1] * (K - 1) + [len(repeats["start"])], orig=a["seq"].encode())
    with pytest.raises(MirgeAmdError):
        predict.write_trimmed_clusters(str(tmp_path / "bad"), "smp", names, cl, t, repeats)
    with pytest.raises(ValueError):
        predict.write_trimmed_clusters(str(tmp_path / "bad"), "smp", names, cl, dict(t, flag=[1] * (K - 1)), repeats)
    with pytest.raises(ValueError):
        predict.write_trimmed_clusters(str(tmp_path / "bad"), "smp", names, cl, dict(t, orig=b"ACGT"), repeats)
    assert not any(os.path.exists(str(tmp_path / "bad") + sfx) for sfx in SUFFIXES)
    cl_bad = dict(cl, members=[len(names)] * len(members))     # a member that is no read: an error, not a crash
    with pytest.raises(MirgeAmdError):
        predict.write_trimmed_clusters(str(tmp_path / "bad2"), "smp", names, cl_bad, dict(t, rep=[-1] * K), repeats)


def test_load_repeats(native_lib, tmp_path):
    from mirge_amd import predict
    parts = genome(["chr2", "chr1", "scaffold_3"])
    empty = predict.load_repeats(str(tmp_path / "nothing_here.tsv"), parts)
    assert empty["rep_off"].tolist() == [0, 0, 0, 0] and len(empty["start"]) == 0 and empty["names"] == []
    assert predict.load_repeats(None, parts)["rep_off"].tolist() == [0, 0, 0, 0]
    f = tmp_path / "rep.tsv"
    f.write_text("chr\tstart\tend\tname\n# a comment\nchr1\t900\t950\tAlu\nchr1\t100\t90\tL1\nchrUn\t5\t9\tnot_there\n"
                 "chr2\t4294967295\t0\tedge\nchr1\t900\t901\tMIR\n\nchr1\t100\t300\tAlu\n")
    r = predict.load_repeats(str(f), parts)
    assert r["rep_off"].tolist() == [0, 1, 5, 5]
    assert r["start"].tolist() == [4294967295, 100, 100, 900, 900] and r["end"].tolist() == [0, 90, 300, 950, 901]
    assert [r["names"][k] for k in r["name_id"]] == ["edge", "L1", "Alu", "Alu", "MIR"] and "not_there" not in r["names"]
    assert r["start"].dtype == r["end"].dtype == r["rep_off"].dtype == r["name_id"].dtype == np.uint32 and r["parts"] is parts
    for bad in ("chr1\t10\t20\n", "chr1\tten\t20\tx\n", "chr1\t-1\t20\tx\n", "chr1\t1\t4294967296\tx\n"):
        f.write_text("chr1\t1\t2\tok\n" + bad)
        with pytest.raises(ValueError, match="line 2"):
            predict.load_repeats(str(f), parts)
    assert predict.repeats_path("/libs", "human") == os.path.join("/libs", "human", "annotation.Libs", "human_genome_repeats.tsv")


def test_parser_options_and_their_defaults():
    from mirge_amd import cli
    base = ["annotate", "-s", "a.fastq", "-lib", "libs", "-sp", "human", "-o", "out"]
    a = cli.build_parser().parse_args(base)
    assert a.clusterSeqLenCutoff == "30" and a.novel_trim is False and a.novel_clusters is False
    a = cli.build_parser().parse_args(base + ["--novel-clusters"])
    assert a.novel_clusters is True and a.novel_trim is False
    a = cli.build_parser().parse_args(base + ["--novel-trim", "-clc", "28"])
    assert a.novel_trim is True and a.clusterSeqLenCutoff == "28"
    assert (a.mapping_loc, a.seedLength, a.overlapLenCutoff) == ("3", "25", "14")


def test_python_entry_points_exist_with_the_documented_defaults():
    import inspect
    from mirge_amd import predict
    from mirge_amd.engine import Engine
    assert inspect.signature(Engine.cluster_valid).parameters["keep_device"].default is False
    assert inspect.signature(predict.map_and_cluster).parameters["trim"].default is None
    assert inspect.signature(predict.map_and_cluster_reads).parameters["trim"].default is None
    assert callable(Engine.predict_trim) and callable(predict.trim_clusters)
