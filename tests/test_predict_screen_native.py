"""Predict mode's screening of the folded candidates without a GPU: the model (tests/predict_screen_model.py) and the host
path of mirge_amd.predict against the reference's own results (tests/golden/predict_screen.json: direct calls of
getPrunedPrecusor / featuresInPrecusor and whole worlds), the stand-in folder's output shape, the native `.str` reader, the
pruned FASTA and the table writer on the fixture's texts, and the options."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import predict_screen_cases as cases
from tests import predict_screen_model as model

GOLD = cases.golden()
WORLDS, CASES = GOLD["worlds"], GOLD["cases"]
TABLE = "unmapped_mirna_smp_vs_representative_seq_modified_selected_sorted_features.tsv"


def model_result(seq, structure, mirnas):
    try:
        pruned = model.prune_slice(seq, structure, mirnas)
    except IndexError as e:
        pruned = {"error": type(e).__name__}
    f = model.features(seq, structure, mirnas, -1.5)
    feat = None if f is None else [f["hairpin_count"], f["binding_count"], f["interior_count"], f["arm"], f["apical"], f["arms"], f["stem_len"],
                                   f["ugu"], f["mfe"], f["pair_state"], f["percent"], f["bindings"]]
    return pruned, feat


def test_fixture_holds_what_it_must():
    assert [w["name"] for w in WORLDS] == ["main", "mapped", "hand_empty", "screen_hand"]
    assert {"not_good", "good_down_only", "good_both", "good_up_only", "all_null", "four_candidates_neighbour_chosen", "mfe_tie",
            "retained_both_arms", "retained_arm5_only", "retained_arm3_only"} <= set(WORLDS[3]["holds"])
    assert len(CASES) == 1500 and os.path.getsize(cases.GOLDEN) < 500000
    lengths = {len(c[0]) for c in CASES}
    assert {1, 63, 64, 65, 255, 256, 257} <= lengths
    assert any(c[3] is None for c in CASES) and any(c[4] is None for c in CASES) and any(len(c[2]) == 2 for c in CASES)
    assert WORLDS[3]["features"].endswith(" \t\n")   # (trailing white space: the writer strips as line.strip() does)


def test_model_reproduces_every_case():
    for seq, structure, mirnas, pruned, feat in CASES:
        assert model_result(seq, structure, mirnas) == (pruned, feat), (seq, structure, mirnas)


def test_host_path_reproduces_every_case():
    from mirge_amd import predict
    for seq, structure, mirnas, pruned, feat in CASES:
        cut = predict.host_prune(seq, structure, mirnas)
        assert (None if cut is None else seq[cut[0]:cut[1]]) == pruned, (seq, structure, mirnas)
        row = predict.host_screen_features(seq, structure, mirnas)
        if feat is None:
            assert row is None
            continue
        want = cases.row_of(seq, structure, mirnas)
        want[0] = 1
        assert row == want, (seq, structure, mirnas)
        # and against the reference's own numbers, not only the model's layout of them
        arms = {cases.ARMS[row[4]]: [row[6], row[7]]}
        if row[8] >= 0:
            arms[cases.ARMS[row[8]]] = [row[9], row[10]]
        assert [row[1], row[2], row[3], cases.ARMS[row[4]], row[5], arms, row[11], "Yes" if row[12] else "No"] == feat[:8]
        assert (row[13] / float(row[14]) if row[14] else 0) == feat[10] and row[13] == feat[11]


HOST_CASES = 24   # of the fixture: the 8 of length 257 and the 16 with ten or more stems or hairpins


def test_exactly_the_cases_built_for_it_take_the_host_path():
    """The condition, from the loop model alone; the GPU test holds the kernels' state word against it."""
    host = [c for c in CASES if cases.takes_host_path(c[0], c[1])]
    assert len(host) == HOST_CASES and sum(len(c[0]) == 257 for c in host) == 8
    for seq, structure, _, _, _ in host:
        hairpins, _, stems = model.elements(structure)
        assert len(seq) == 257 or len(stems) >= 10 or len(hairpins) >= 10
    assert {(len(model.elements(c[1])[2]), len(model.elements(c[1])[0])) for c in host if len(c[0]) < 100} >= {(10, 1), (11, 1), (10, 10), (11, 11)}


@pytest.mark.parametrize("w", WORLDS, ids=lambda w: w["name"])
def test_model_reproduces_the_worlds(w):
    assert model.screen(w["features"], w["str"], cases.fold_many) == w["table"]


def test_model_refuses_what_the_reference_dies_of():
    header, rows = model.read_features(WORLDS[3]["features"])
    good = [r for r in rows if r[3] == "Good"]
    with pytest.raises(IndexError, match="line 0"):
        model.candidates([good[1]])            # a neighbour before the first line
    with pytest.raises(IndexError):
        model.candidates([(good[0][0], "x", "ACGU", "Good", 10000, 10000)])
    with pytest.raises(model.StructureError):
        model.elements("((..))")
    with pytest.raises(model.StructureError):
        model.pair_table("(()")


def test_stand_in_folder_writes_rnafold_shaped_records():
    name = ">smp:miRCluster_7_22:chr10:120_141+:precusor_1"
    text = "%s\nGGGGGGGGAAAACCCCCCCC\n>b\nGGGAAAACCC\n>c\nGGGGAAAACCCC\n" % name
    out = subprocess.run([sys.executable, cases.STANDIN, "--noPS", "--noLP"], input=text, capture_output=True, text=True, check=True).stdout
    lines = out.split("\n")
    assert lines[0] == name[:42] and lines[1] == "GGGGGGGGAAAACCCCCCCC"
    # (a helix of three is not admissible: nothing pairs)
    assert lines[2] == "((((((((....)))))))) ( -5.60)" and lines[5] == ".......... (  0.00)" and lines[8] == "((((....)))) ( -2.80)"
    assert [r[3] for r in model.parse_str(out)] == [-5.6, 0.0, -2.8]
    big = subprocess.run([sys.executable, cases.STANDIN], input=">x\n" + "GC" * 20 + "\n", capture_output=True, text=True, check=True).stdout
    assert "(-" in big.split("\n")[2]        # the other energy shape: no blank behind the bracket
    assert os.access(cases.STANDIN, os.X_OK)


# ------------------------------------------------------------------------------------------------- the native host code
@pytest.mark.parametrize("w", WORLDS, ids=lambda w: w["name"])
def test_str_reader_gives_the_records_as_arrays(native_lib, tmp_path, w):
    from mirge_amd import predict
    path = str(tmp_path / "w.str")
    with open(path, "w") as fh:
        fh.write(w["str"])
    records = model.parse_str(w["str"])
    off, seq, structure, mfe = predict.read_str_file(path, len(records))
    assert off.tolist() == np.cumsum([0] + [len(r[1]) for r in records]).tolist()
    assert seq.decode() == "".join(r[1] for r in records) and structure.decode() == "".join(r[2] for r in records)
    assert mfe.tolist() == [r[3] for r in records]


def test_str_reader_parses_both_energy_shapes_and_refuses_a_wrong_count(native_lib, tmp_path):
    from mirge_amd import predict
    from mirge_amd._native import MirgeAmdError
    text = (">a\nGGGAAAACCC\n(((....))) (-12.30)\n>b\nGGGAAAACCC\n(((....))) ( -2.30)\n>c\nAAAA\n.... (  0.00)\n"
            ">d\nAAAA\n....\n>e\nAAAA\n.... (x.y)\n>f\nAAAA\n.... ( zz)\r\n")
    path = str(tmp_path / "e.str")
    with open(path, "w", newline="") as fh:
        fh.write(text)
    off, seq, structure, mfe = predict.read_str_file(path, 6)
    assert mfe.tolist() == [-12.3, -2.3, 0.0, 0.0, 0.0, 0.0] == [r[3] for r in model.parse_str(text)]
    assert structure.decode() == "(((....)))(((....)))" + "...." * 4
    with pytest.raises(MirgeAmdError, match=r"6 folded records .* 7 sequences"):
        predict.read_str_file(path, 7)
    with open(path, "a") as fh:
        fh.write(">g\nAAAA\n")
    with pytest.raises(MirgeAmdError, match=r"7 folded records \(20 lines\) for the 7 sequences"):
        predict.read_str_file(path, 7)
    with open(path, "w") as fh:
        fh.write(">a\nGGGAAAACCC\n(((...))) (-1.00)\n")
    with pytest.raises(MirgeAmdError, match="structure's length"):
        predict.read_str_file(path, 1)
    with pytest.raises(MirgeAmdError):
        predict.read_str_file(str(tmp_path / "none.str"), 0)


def test_pruned_fasta_names_the_kept_strings(native_lib, tmp_path):
    from mirge_amd import predict
    off, seq = cases.blob(["ACGU", "", "GGG", "U"])
    path = str(tmp_path / "p.fa")
    assert predict.write_pruned_fasta(path, off, seq, [1, 0, 1, 1]) == 3
    assert open(path).read() == ">c0\nACGU\n>c2\nGGG\n>c3\nU\n"
    with pytest.raises(ValueError, match="close at"):
        predict.write_pruned_fasta(path, off[:-1], seq, [1, 0, 1])


@pytest.mark.parametrize("threads,block", [(1, None), (4, 3)])
@pytest.mark.parametrize("w", WORLDS, ids=lambda w: w["name"])
def test_table_writer_reproduces_the_worlds(native_lib, tmp_path, monkeypatch, w, threads, block):
    from mirge_amd import predict
    a = cases.world_arrays(w)
    assert not (a["feat"][:, 0] == 2).any() and not (a["status"] == 2).any()      # no world sends a candidate to the host
    if block is not None:
        monkeypatch.setenv("MIRGE_AMD_SCREEN_BLOCK_LINES", str(block))
    features, out = str(tmp_path / TABLE), str(tmp_path / (TABLE[:-4] + model.UPDATED_SUFFIX))
    with open(features, "w") as fh:
        fh.write(w["features"])
    lines = predict.write_screened_features(features, out, a["best"], a["feat"], a["p_off"], a["p_seq"], a["p_str"], a["p_mfe"], threads=threads)
    assert lines == a["n"] and open(out).read() == w["table"]


def test_table_writer_refuses_arrays_that_contradict_the_file(native_lib, tmp_path):
    from mirge_amd import predict
    from mirge_amd._native import MirgeAmdError
    w = WORLDS[3]
    a = cases.world_arrays(w)
    features, out = str(tmp_path / TABLE), str(tmp_path / "out.tsv")
    with open(features, "w") as fh:
        fh.write(w["features"] + "one\tline\tmore\n")
    with pytest.raises(MirgeAmdError, match="lines below the header"):
        predict.write_screened_features(features, out, a["best"], a["feat"], a["p_off"], a["p_seq"], a["p_str"], a["p_mfe"])
    with open(features, "w") as fh:
        fh.write(w["features"])
    feat = a["feat"].copy()
    line = int(np.flatnonzero(a["best"] >= 0)[0])
    feat[4 * line + a["best"][line], 0] = 0
    with pytest.raises(MirgeAmdError, match="line %d: the chosen candidate has no feature row" % line):
        predict.write_screened_features(features, out, a["best"], feat, a["p_off"], a["p_seq"], a["p_str"], a["p_mfe"])
    assert not os.path.exists(out)
    with pytest.raises(ValueError, match="must match"):
        predict.write_screened_features(features, out, a["best"][:-1], a["feat"], a["p_off"], a["p_seq"], a["p_str"], a["p_mfe"])


# ------------------------------------------------------------------------------------------------------------- options
def test_novel_screen_implies_the_earlier_stages_and_needs_a_fold_command(tmp_path, capsys):
    import inspect
    from mirge_amd import cli, predict
    base = ["annotate", "-s", "x.fastq", "-lib", "l", "-sp", "syn"]
    args = cli.build_parser().parse_args(base + ["--novel-screen"])
    assert args.novel_screen and not args.novel_precursors and cli.novel_stages(args) == (True, True, True, True)
    assert not cli.build_parser().parse_args(base).novel_screen
    args = cli.build_parser().parse_args(base + ["--novel-screen", "-pr", "/somewhere", "--fold-cmd", cases.STANDIN])
    assert args.rnafoldBinary == "/somewhere" and args.fold_cmd == cases.STANDIN
    assert predict.resolve_fold_cmd("/somewhere", cases.STANDIN) == os.path.abspath(cases.STANDIN)    # --fold-cmd overrides -pr
    os.symlink(cases.STANDIN, str(tmp_path / "RNAfold"))
    assert predict.resolve_fold_cmd(str(tmp_path), None) == str(tmp_path / "RNAfold")
    with pytest.raises(ValueError, match=r"^RNAfold can't be found in /nowhere\. Please check it\.$"):
        predict.resolve_fold_cmd("/nowhere", None)
    with pytest.raises(ValueError, match=r"^RNAfold can't be found in None\. Please check it\.$"):
        predict.resolve_fold_cmd(None, None)
    for fn in (predict.map_and_cluster, predict.map_and_cluster_reads):
        assert inspect.signature(fn).parameters["screen"].default is False
    with pytest.raises(ValueError, match="screen needs precursors"):
        predict.map_and_cluster(None, str(tmp_path / "none.fa"), "g", 3, 25, 14, str(tmp_path / "x"), screen=True)
    with pytest.raises(SystemExit):
        predict.main(["clusters", "g", "r.fa", "-o", str(tmp_path / "x"), "--trim", "--remap", "--features", "--screen"])
    assert predict.main(["clusters", "g", "r.fa", "-o", str(tmp_path / "x"), "--trim", "--remap", "--features", "--precursors", "--screen"]) == 1
    assert "RNAfold can't be found in None. Please check it." in capsys.readouterr().err


def test_annotate_novel_screen_without_a_fold_command_exits_1_before_any_work(tmp_path, capsys):
    from mirge_amd import cli
    args = cli.build_parser().parse_args(["annotate", "-s", str(tmp_path / "x.fastq"), "-lib", str(tmp_path), "-sp", "syn", "-o", str(tmp_path),
                                          "--novel-screen", "-pr", str(tmp_path / "bin")])
    with pytest.raises(SystemExit) as e:
        cli.annotate_main(args)
    assert e.value.code == 1
    assert "RNAfold can't be found in %s. Please check it." % (tmp_path / "bin") in capsys.readouterr().err
    assert os.listdir(str(tmp_path)) == []     # nothing was made: the check comes first


def test_fold_command_starts_the_executable_without_a_shell(tmp_path):
    from mirge_amd import predict
    fasta, out = str(tmp_path / "in put;.fa"), str(tmp_path / "out.str")
    with open(fasta, "w") as fh:
        fh.write(">a\nGGGGAAAACCCC\n")
    predict.fold_command(cases.STANDIN)(fasta, out)
    assert open(out).read() == ">a\nGGGGAAAACCCC\n((((....)))) ( -2.80)\n"
    with pytest.raises(OSError):
        predict.fold_command("/bin/false")(fasta, out)
