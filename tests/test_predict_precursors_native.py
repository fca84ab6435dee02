"""Predict mode's precursor candidates without a GPU: the model (tests/predict_precursors_model.py) against the golden files
of the reference's get_precursors.py (tests/golden/predict_precursors.json), the native writer (mrg_write_precursors) fed the
model's arrays on 1 and 4 threads and in blocks of 3 records, its refusals, rename_str_file against the reference's
renameStrFile, and the options' parsing."""
import os

import numpy as np
import pytest

from tests import predict_precursors_cases as cases
from tests import predict_precursors_model as model

GOLD = cases.golden()
WORLDS = GOLD["worlds"]
WANTED = {"plus", "minus", "overhang_plus", "overhang_minus", "unstable_plus", "unstable_minus", "first_clamped_at_0",
          "both_clamped_at_0", "second_beyond_end", "both_beyond_end", "n_run_inside", "starts_in_n_run", "ends_in_n_run",
          "index_order_is_not_name_order", "empty_table"}


@pytest.mark.parametrize("w", WORLDS, ids=lambda w: w["name"])
def test_model_reproduces_the_golden_files(w):
    assert model.run(w["features"], w["chromosomes"]) == w["precursors"]
    assert w["precursors"].count(">") == 2 * len(model.lines(w["features"]))


def test_golden_worlds_hold_every_case():
    assert [w["name"] for w in WORLDS] == ["main", "mapped", "empty", "hand", "hand_empty"]
    assert WANTED - {"empty_table"} <= set(WORLDS[3]["holds"]) and "empty_table" in WORLDS[4]["holds"]
    assert WORLDS[2]["precursors"] == WORLDS[4]["precursors"] == ""
    assert os.path.getsize(cases.GOLDEN) < 60000


def test_model_skips_a_repeated_name_and_refuses_a_window_before_the_chromosome():
    w = WORLDS[3]
    rows = w["features"].split("\n")
    twice = "\n".join(rows[:2] + [rows[1]] + rows[2:])
    assert model.run(twice, w["chromosomes"]) == w["precursors"]
    assert model.windows(1, 1, 100) == [(0, 21), (0, 71)]
    with pytest.raises(ValueError, match="first base"):
        model.windows(-30, -20, 100)
    assert model.windows(500, 520, 100) == [(100, 100), (100, 100)]   # (an empty slice: an empty line)


def write_world(tmp_path, w, threads=None, block=None, monkeypatch=None, **change):
    from mirge_amd import predict
    a = cases.Arrays(w["features"], w["chromosomes"])
    parts, index = a.indexes()
    path = str(tmp_path / ("t" + model.SUFFIX))
    if block is not None:
        monkeypatch.setenv("MIRGE_AMD_PRECURSOR_BLOCK_RECORDS", str(block))
    args = dict(cl_entry=a.cl["entry"], group_cluster=a.group_cluster, rec=a.rec)
    args.update(change)
    records, nbytes = predict.write_precursors(path, parts, index, args["cl_entry"], args["group_cluster"], args["rec"], threads=threads)
    text = open(path).read()
    assert records == text.count(">") and nbytes == len(text)
    return text


@pytest.mark.parametrize("threads,block", [(1, None), (4, None), (4, 3), (1, 3)])
@pytest.mark.parametrize("w", WORLDS, ids=lambda w: w["name"])
def test_native_writer_reproduces_the_golden_files(native_lib, tmp_path, monkeypatch, w, threads, block):
    assert write_world(tmp_path, w, threads, block, monkeypatch) == w["precursors"]


def test_native_writer_refuses_arrays_that_do_not_fit(native_lib, tmp_path):
    from mirge_amd._native import MirgeAmdError
    w = WORLDS[3]
    a = cases.Arrays(w["features"], w["chromosomes"])
    r = a.rec
    with pytest.raises(ValueError, match="must match"):
        write_world(tmp_path, w, rec=dict(r, rec_lo=r["rec_lo"][:-1]))
    with pytest.raises(ValueError, match="must match"):
        write_world(tmp_path, w, rec=dict(r, rec_off=r["rec_off"][:-1]))
    with pytest.raises(ValueError, match="close at"):
        write_world(tmp_path, w, rec=dict(r, seq=r["seq"] + b"A"))
    with pytest.raises(ValueError, match="retained clusters"):
        write_world(tmp_path, w, cl_entry=a.cl["entry"][:-1])
    shifted = r["rec_off"].copy()
    shifted[3] += 1
    swapped = r["rec_group"].copy()
    swapped[[0, 2]] = swapped[[2, 0]]
    beyond = r["rec_hi"].copy()
    beyond[0] = 10 ** 6
    for bad in (dict(rec=dict(r, rec_off=shifted)), dict(rec=dict(r, rec_group=swapped)), dict(rec=dict(r, rec_hi=beyond)),
                dict(rec=dict(r, rec_group=np.full_like(r["rec_group"], a.n_groups))),
                dict(rec=dict(r, rec_group=np.concatenate([r["rec_group"][:2], r["rec_group"][:2], r["rec_group"][4:]]))),
                dict(rec={k: (v[:-1] if k != "seq" else v[:int(r["rec_off"][-2])]) for k, v in r.items()}),     # an odd count
                dict(group_cluster=np.full_like(a.group_cluster, a.n_groups)), dict(cl_entry=a.cl["entry"] + 2)):
        with pytest.raises(MirgeAmdError) as e:
            write_world(tmp_path, w, **bad)
        assert e.value.code == -1
    assert not os.path.exists(str(tmp_path / ("t" + model.SUFFIX)))


def test_rename_str_file_is_the_reference(tmp_path):
    from mirge_amd import predict
    g = GOLD["rename"]
    (tmp_path / "in.fa").write_text(g["fasta"])
    (tmp_path / "in.str").write_text(g["str"])
    assert predict.rename_str_file(str(tmp_path / "in.fa"), str(tmp_path / "in.str"), str(tmp_path / "out.str")) == 3
    assert (tmp_path / "out.str").read_text() == g["renamed"]
    assert g["renamed"] != g["str"] and g["renamed"].count(":precusor_") == 3
    (tmp_path / "short.fa").write_text(g["fasta"][:g["fasta"].index(">", 1)])
    with pytest.raises(ValueError, match="folded records"):
        predict.rename_str_file(str(tmp_path / "short.fa"), str(tmp_path / "in.str"), str(tmp_path / "out2.str"))


def test_options_parse_and_imply_the_earlier_stages(tmp_path):
    from mirge_amd import cli, predict
    args = cli.build_parser().parse_args(["annotate", "-s", "x.fastq", "-lib", "l", "-sp", "syn", "--novel-precursors"])
    assert args.novel_precursors and not args.novel_features
    assert cli.novel_stages(args) == (True, True, True, True)
    args = cli.build_parser().parse_args(["annotate", "-s", "x.fastq", "-lib", "l", "-sp", "syn"])
    assert not args.novel_precursors and cli.novel_stages(args) == (False, False, False, False)
    with pytest.raises(SystemExit):
        predict.main(["clusters", "g", "r.fa", "-o", str(tmp_path / "x"), "--trim", "--remap", "--precursors"])
    with pytest.raises(ValueError, match="precursors needs features"):
        predict.map_and_cluster(None, str(tmp_path / "none.fa"), "g", 3, 25, 14, str(tmp_path / "x"), precursors=True, features=False)
    with pytest.raises(ValueError, match="precursors needs features"):
        predict.map_and_cluster_reads(None, None, None, None, "g", 3, 25, 14, str(tmp_path / "x"), precursors=True)


def test_no_feature_line_writes_an_empty_file(tmp_path):
    from mirge_amd import predict
    stem = str(tmp_path / "unmapped_mirna_smp")
    got = predict.cluster_precursors(None, dict(lines=0), dict(clusters={}), [], stem)
    assert got["records"] == 0 and got["n_written"] == 0
    assert open(stem + predict.REMAP_SUFFIX[:-4] + "_features_precusor.fa").read() == ""
