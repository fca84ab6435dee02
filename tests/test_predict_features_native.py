"""Predict mode's cluster feature table without a GPU: the model (tests/predict_features_model.py) against the golden files
of the reference's generate_featureFiles.py and readCluster.py (tests/golden/predict_features.json), the native writer
(mrg_write_predict_features) fed the model's arrays on 1 and 4 threads and in blocks of 3 groups, the float printing, the
integer form of the 0.8 test, and the refusals that precede a device call."""
import os

import numpy as np
import pytest

from tests import predict_features_cases as cases
from tests import predict_features_model as model

WORLDS = cases.golden_worlds()
WANTED = {"sum_9", "sum_10", "members_2", "members_3", "start_20", "start_21", "end_at_limit", "end_below_limit",
          "overhang_head_and_tail", "pass2_cut_mismatch", "member_twice", "ratio_4_5", "ratio_7_9", "ratio_8_10", "column_tie",
          "no_stable_column", "head_below_3", "head_from_3", "tail_add_below_6", "tail_add_from_6", "minus_cluster",
          "stable_length_6", "stable_length_7", "chromosome_with_1", "chromosome_with_2", "chromosome_with_4", "distance_8",
          "distance_9", "distance_44", "distance_45", "unequal_strands", "chr10_before_chr2", "template_n_later_column",
          "tied_alignment", "member_with_n", "mapped_name", "no_surviving_group"}


@pytest.mark.parametrize("w", WORLDS, ids=lambda w: w["name"])
def test_model_reproduces_the_golden_files(native_lib, w):
    feats, clus, info = model.run(w["table"], w["chromosomes"], w["table_name"])
    assert feats == w["features"]
    assert clus == w["cluster"]
    assert info["seen"] >= info["passed"] >= clus.count("Cluster Name: ")


def test_golden_worlds_hold_every_case():
    assert WANTED <= set(h for w in WORLDS for h in w["holds"])
    assert os.path.getsize(cases.GOLDEN) < 100000


def write_world(tmp_path, w, mode, threads=None, block=None, monkeypatch=None):
    """mrg_write_predict_features over the model's arrays.  mode "diag": every group from (diagonal, read) but those with
    an N or a dash inside a row; "text": every group from its text."""
    from mirge_amd import predict
    a = cases.Arrays(w["table"], w["chromosomes"])
    exp = a.expected(w["table"])
    parts, index = a.indexes()
    words, lens, nmask = a.packed()
    texts = dict(exp["rows_text"])
    if mode == "diag":
        texts = {g: t for g, t in texts.items() if "N" in t or any("-" in row.strip("-") for row in t.split("\n"))}
    res = dict(exp, n_groups=a.n_groups, row_read=a.row_read, group_off=a.group_off, group_cluster=a.group_cluster)
    path = str(tmp_path / w["table_name"])
    if block is not None:
        monkeypatch.setenv("MIRGE_AMD_FEATURE_BLOCK_GROUPS", str(block))
    blocks, lines = predict.write_predict_features(path, parts, index, a.cl, a.kept_seq_off, a.kept_orig, words, lens, nmask, a.counts,
                                                   res, texts, threads=threads)
    feats, clus = open(path[:-4] + "_features.tsv").read(), open(path[:-4] + "_cluster.txt").read()
    assert blocks == clus.count("Cluster Name: ") and lines == max(feats.count("\n") - 1, 0)
    return feats, clus, len(texts)


@pytest.mark.parametrize("mode", ["diag", "text"])
@pytest.mark.parametrize("w", WORLDS, ids=lambda w: w["name"])
def test_native_writer_reproduces_the_golden_files(native_lib, tmp_path, w, mode):
    feats, clus, n_text = write_world(tmp_path, w, mode)
    assert feats == w["features"]
    assert clus == w["cluster"]
    if w["name"] == "main":
        assert n_text == (1 if mode == "diag" else 21)   # (the group with an N; every group that passes the filter)


@pytest.mark.parametrize("threads,block", [(1, None), (4, None), (4, 3), (1, 3)])
def test_native_writer_bytes_do_not_depend_on_threads_or_blocks(native_lib, tmp_path, monkeypatch, threads, block):
    w = WORLDS[0]
    feats, clus, _ = write_world(tmp_path, w, "diag", threads=threads, block=block, monkeypatch=monkeypatch)
    assert feats == w["features"] and clus == w["cluster"]


def test_float_text_agrees_with_python2_str():
    from mirge_amd.report import py2_float_str
    for den in range(1, 61):
        for num in range(0, 61):
            q = float(num) / den
            assert model.py2_str(q) == py2_float_str(q)
    assert model.py2_str(0) == "0" and model.py2_str(0.0) == "0.0" and model.py2_str(1.0) == "1.0"
    assert model.py2_str(2.0 / 3) == "0.666666666667" and model.py2_str(None) == "None" and model.py2_str(1e-5) == "1e-05"


def test_integer_ratio_test_is_the_float_one():
    from mirge_amd import predict
    for s in range(1, 2001):
        for c in range(0, s + 1):
            assert model.ratio_reached(c, s) == (float(c) / s >= 0.8), (c, s)
    rng = np.random.default_rng(80)
    for s in rng.integers(1, 2 ** 40, 100000):
        s = int(s)
        for c in (int(rng.integers(0, s + 1)), (4 * s) // 5, (4 * s + 4) // 5, max((4 * s) // 5 - 1, 0)):
            assert model.ratio_reached(c, s) == predict.ratio_reached(c, s) == (float(c) / s >= 0.8), (c, s)


def test_host_group_is_the_model(native_lib):
    """predict.host_group, the route of the groups the device leaves, against the model on every golden group."""
    from mirge_amd import predict
    for w in WORLDS:
        a = cases.Arrays(w["table"], w["chromosomes"])
        exp = a.expected(w["table"])
        for g, text in exp["rows_text"].items():
            members = a.row_read[a.group_off[g]:a.group_off[g + 1]]
            rows, numbers = predict.host_group(a.cseqs[int(a.group_cluster[g])], [a.seqs[int(r)] for r in members], a.counts[members])
            assert "\n".join(rows) == text
            if not exp["valid"][g]:
                assert numbers is None
                continue
            assert (numbers["H"], numbers["T"], numbers["head"], numbers["tail"]) == tuple(int(x) for x in exp["frame"][g])
            assert numbers["exact"] == int(exp["exact"][g]) and numbers["nine"] == [int(x) for x in exp["nine"][g]]


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_before_any_device_call(native_lib, tmp_path):
    from mirge_amd import predict
    from mirge_amd._native import MirgeAmdError
    w = WORLDS[0]
    a = cases.Arrays(w["table"], w["chromosomes"])
    exp = a.expected(w["table"])
    parts, index = a.indexes()
    words, lens, nmask = a.packed()
    res = dict(exp, n_groups=a.n_groups, row_read=a.row_read, group_off=a.group_off, group_cluster=a.group_cluster)
    texts = exp["rows_text"]

    def call(path=None, res=res, cl=a.cl, texts=texts, counts=a.counts):
        path = path or str(tmp_path / w["table_name"])
        return predict.write_predict_features(path, parts, index, cl, a.kept_seq_off, a.kept_orig, words, lens, nmask, counts, res, texts)
    with pytest.raises(ValueError, match="mapped_mirna"):
        call(path=str(tmp_path / "mapped_mirna_smp_vs_representative_seq_modified_selected_sorted.tsv"))
    with pytest.raises(ValueError, match="mapped_mirna"):
        model.run(w["table"], w["chromosomes"], "mapped_mirna_x.tsv")
    with pytest.raises(ValueError, match="must match"):
        call(counts=a.counts[:-1])
    with pytest.raises(ValueError, match="do not fit"):
        call(res=dict(res, nb_t=res["nb_t"][:-1]))
    with pytest.raises(ValueError, match="text for group"):
        call(texts={a.n_groups: "A"})
    # arrays that contradict each other: refused by the writer before a file is opened
    for bad in (dict(res, order=np.array([a.n_groups], np.uint32)), dict(res, order=np.array([0, 0], np.uint32)),
                dict(res, group_off=np.concatenate([a.group_off[:-1], [a.group_off[-1] + 1]]).astype(np.uint32)),
                dict(res, row_read=np.full_like(a.row_read, len(a.names))),
                dict(res, frame=np.array(exp["frame"]) + np.array([0, 0, 200, 0], np.int32))):
        with pytest.raises(MirgeAmdError) as e:
            call(res=bad)
        assert e.value.code == -1
    assert not os.path.exists(str(tmp_path / w["table_name"])[:-4] + "_features.tsv")
    # a template range that leaves its chromosome names the cluster
    g = int(exp["order"][0])
    c = int(a.group_cluster[g])
    moved = dict(a.cl, start=a.cl["start"].copy(), end=a.cl["end"].copy())
    moved["start"][c], moved["end"][c] = 2, 2 + len(a.cseqs[c]) - 1
    with pytest.raises(ValueError, match="leaves its chromosome") as e:
        call(cl=moved)
    assert a.cnames[c] in str(e.value)
    d = [x for x in exp["info"]["groups"] if x["cluster"] == a.cnames[c]][0]
    with pytest.raises(ValueError, match="leaves its chromosome"):   # the model says the same
        model.nine_columns([2, int(moved["end"][c]), a.cnames[c], a.cseqs[c]], d["rows"], d["counts"], d["head"], d["tail"], "ACGT" * 100)
    # the routes' own argument checks
    with pytest.raises(ValueError, match="features needs remap"):
        predict._map_cluster_write(None, None, None, None, None, "x", 3, 25, 14, "x", False, None, trim=(None, 30), remap=False, features=True)
    with pytest.raises(ValueError, match="retained_clusters"):
        predict.cluster_features(None, None, a.counts, dict(kept=a.kept), dict(n_rows=1), parts, str(tmp_path / "x"))


def test_no_group_writes_the_partial_header(native_lib, tmp_path):
    from mirge_amd import predict
    stem = str(tmp_path / "unmapped_mirna_smp")
    trim = dict(kept=np.zeros(0, np.uint32), kept_seq_off=np.zeros(1, np.uint64), kept_orig=b"",
                clusters=dict(entry=[], strand=[], start=[], end=[]))
    got = predict.cluster_features(None, None, np.zeros(0, np.uint32), trim, dict(n_rows=0), [], stem)
    assert got["written"] == 0 and got["seen"] == 0
    table = stem + predict.REMAP_SUFFIX
    assert open(table[:-4] + "_features.tsv").read() == model.HEADER_HEAD
    assert open(table[:-4] + "_cluster.txt").read() == ""
