"""Predict mode's classification on the GPU (-m gpu): mrg_predict_svm against the rule (tests/predict_model_model.py) with
guard words behind every output -- hand-made models over the feature counts of every register bucket and support-vector
counts around the LDS tile (64), row counts around the workgroup (64), rows so far away that every kernel value underflows,
decision values so large that the clip applies, inputs of every coupling round count, a kept row whose larger probability is
class -1's, permuted rows bit for bit --, the fixture's worlds end to end through predict.classify_candidates against the
reference's five files, and `predict clusters --classify` and `annotate --novel-predict` over the files the same run wrote.

Decision values must agree within T = 4 2^-53 n_sv sum|coef| of the model at hand (the worst case of adding the terms in
another order), probabilities within T max(1, |A| / 4)."""
import os
import sys

import numpy as np
import pytest

from tests import predict_model_cases as cases
from tests import predict_model_model as rule

pytestmark = pytest.mark.gpu

GOLD = cases.golden()
WORLDS = {w["name"]: w for w in GOLD["worlds"]}
NAMELIST = GOLD["namelist"]
GUARD = 64
FILL = 0x5A
TILE = 64      # support vectors of an LDS tile (csrc/predict_svm.hpp: kSvmTile)


@pytest.fixture(scope="module")
def engine(native_lib):
    from mirge_amd.engine import Engine
    eng = Engine(0)
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def model():
    return cases.fixture_model()


@pytest.fixture(scope="module")
def thousand(model):
    """1000 rows around the fixture model's support vectors and the rule's results for them: computed once, never changed."""
    x = cases.hand_rows(model, 1000, seed=9, noise=cases.NOISE)
    x.setflags(write=False)
    return x, rule.classify(model, x)


def error(engine):
    return (engine._lib.mrg_last_error() or b"").decode()


def call_svm(engine, x, m, expect_error=None, nf=None, n_sv=None):
    """mrg_predict_svm on device buffers with guard words behind pred, dec and prob: dict of host arrays."""
    import torch
    x = np.ascontiguousarray(x, dtype=np.float64)
    nf = m.sv.shape[1] if nf is None else nf
    n_sv = m.sv.shape[0] if n_sv is None else n_sv
    n = x.size // m.sv.shape[1]
    up = lambda a: torch.from_numpy(np.array(a, dtype=np.float64).reshape(-1) if np.size(a) else np.zeros(1)).to(engine.device)
    ins = [up(x), up(m.mean), up(m.scale), up(m.sv), up(m.coef)]
    outs = [torch.from_numpy(np.full(count + GUARD, FILL, dtype=dt)).to(engine.device) for count, dt in ((n, np.int8), (n, np.float64), (2 * n, np.float64))]
    p = lambda t: t.data_ptr()
    rc = engine._lib.mrg_predict_svm(engine._h, n, p(ins[0]), nf, p(ins[1]), p(ins[2]), p(ins[3]), p(ins[4]), n_sv, m.intercept, m.gamma,
                                     m.probA, m.probB, p(outs[0]), p(outs[1]), p(outs[2]), engine._stream_ptr())
    torch.cuda.synchronize()
    host = [t.cpu().numpy() for t in outs]
    for h, count in zip(host, (n, n, 2 * n)):
        assert h[count:].shape[0] == GUARD and (h[count:] == FILL).all()          # the guard words are intact
    if expect_error is not None:
        assert rc == -1 and expect_error in error(engine), error(engine)
        assert all((h == FILL).all() for h in host)
        return None
    assert rc == 0, error(engine)
    return dict(pred=host[0][:n], dec=host[1][:n], prob=host[2][:2 * n].reshape(n, 2))


def agree(m, got, want, rows=None):
    """Labels equal (but where the decision value is within T of 0), decision values within T, probabilities within
    T max(1, |A| / 4)."""
    t = rule.tolerance(m)
    sel = slice(None) if rows is None else rows
    dec, pred, prob = want["dec"][sel], want["pred"][sel], want["prob"][sel]
    assert got["dec"].shape == dec.shape
    if dec.size == 0:
        return True
    assert np.abs(got["dec"] - dec).max() <= t, (np.abs(got["dec"] - dec).max(), t)
    sure = np.abs(dec) > t
    assert (got["pred"][sure] == pred[sure]).all() and set(got["pred"].tolist()) <= {1, -1}
    settled = np.array([not any(abs(e - rule.COUPLING_EPS) <= cases.STOP_MARGIN * rule.COUPLING_EPS for e in err) for err in want["errors"]])[sel]
    assert np.abs(got["prob"] - prob)[settled].max(initial=0.0) <= cases.prob_margin(m, t), (np.abs(got["prob"] - prob)[settled].max(), t)
    assert np.abs(got["prob"].sum(axis=1) - 1.0).max() < 1e-12
    return True


# ------------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize("n_sv", [1, TILE - 1, TILE, TILE + 1, 2959])
@pytest.mark.parametrize("nf", [1, 12, 21, 64])
def test_hand_models(engine, nf, n_sv):
    m = cases.hand_model(nf, n_sv, gamma=1.0 / nf)
    x = cases.hand_rows(m, 65, seed=nf)
    want = rule.classify(m, x)
    assert agree(m, call_svm(engine, x, m), want)


@pytest.mark.parametrize("n_rows", [0, 1, 63, 64, 65, 1000])
def test_row_counts_with_the_fixture_model(engine, model, thousand, n_rows):
    x, want = thousand
    got = call_svm(engine, x[:n_rows], model)
    assert got["pred"].shape == (n_rows,) and agree(model, got, want, slice(0, n_rows))


def test_rows_far_away_get_the_intercept(engine, model):
    x = model.mean + model.scale * np.array([[1e6], [-1e6], [3e4]]) * np.ones((3, model.sv.shape[1]))
    got = call_svm(engine, x, model)
    assert (got["dec"] == model.intercept).all() and (got["pred"] == -1).all()
    want = rule.classify(model, x)
    assert (want["dec"] == model.intercept).all() and agree(model, got, want)


def test_huge_decision_values_are_clipped(engine):
    base = cases.hand_model(3, 8, gamma=0.5)
    for sign in (1.0, -1.0):
        m = base._replace(sv=np.zeros((8, 3)), coef=np.full(8, sign * 10.0), intercept=0.25)
        x = np.tile(m.mean, (5, 1)) + m.scale * np.array([0.0, 0.01, 0.1, 0.5, 30.0])[:, None]
        want = rule.classify(m, x)
        assert want["clipped"][:3].all() and not want["clipped"][4] and abs(want["dec"][0]) > 79
        got = call_svm(engine, x, m)
        assert agree(m, got, want)
        assert (got["prob"][:3] == got["prob"][0]).all() and (want["prob"][:3] == want["prob"][0]).all()   # one clipped value, one result
        assert (got["pred"][:3] == (1 if sign > 0 else -1)).all()


def test_inputs_of_every_coupling_round_count(engine):
    m = cases.hand_model(1, 1, gamma=1.0)._replace(mean=np.zeros(1), scale=np.ones(1), sv=np.zeros((1, 1)), intercept=-2.0)
    x = np.sqrt(np.linspace(0.0, 6.0, 600))[:, None]          # decision values from 8 down to about -2
    want = rule.classify(m, x)
    assert {0, 1, 2} <= set(want["rounds"].tolist())
    got = call_svm(engine, x, m)
    assert agree(m, got, want)
    # without the iteration the numbers are off by thousandths: the pairwise value is not what libsvm returns
    pairwise = np.array([min(max(rule.sigmoid(-f, m.probA, m.probB), rule.MIN_PROB), 1 - rule.MIN_PROB) for f in want["dec"]])
    assert 1e-3 < np.abs(pairwise - got["prob"][:, 0]).max() < 1e-2


def test_a_row_predicted_1_whose_larger_probability_is_class_minus_1s(engine):
    m = cases.hand_model(4, 30, gamma=0.25, prob_b=-3.0)
    x = cases.hand_rows(m, 400, seed=2)
    want = rule.classify(m, x)
    odd = (want["pred"] == 1) & (want["prob"][:, 0] >= rule.CUTOFF)
    assert odd.any()
    got = call_svm(engine, x, m)
    assert agree(m, got, want)
    sure = odd & (np.abs(want["dec"]) > rule.tolerance(m)) & (np.abs(want["prob"][:, 0] - rule.CUTOFF) > 1e-9)
    assert sure.any() and (got["pred"][sure] == 1).all() and (got["prob"][sure, 0] >= rule.CUTOFF).all()


def test_permuted_rows_give_the_same_bits_permuted(engine, model, thousand):
    x, _ = thousand
    first = call_svm(engine, x, model)
    perm = np.random.default_rng(4).permutation(len(x))
    second = call_svm(engine, x[perm], model)
    for key in ("pred", "dec", "prob"):
        assert first[key][perm].tobytes() == second[key].tobytes()
    part = call_svm(engine, x[937:], model)          # another place in the batch, another launch geometry
    for key in ("pred", "dec", "prob"):
        assert first[key][937:].tobytes() == part[key].tobytes()


def test_engine_method_and_refusals(engine, model, thousand):
    x, want = thousand
    res = engine.predict_svm(x[:130], model)
    assert res["pred"].dtype == np.int8 and res["prob"].shape == (130, 2) and agree(model, res, want, slice(0, 130))
    empty = engine.predict_svm(np.zeros((0, 21)), model)
    assert empty["pred"].shape == (0,) and empty["prob"].shape == (0, 2)
    with pytest.raises(ValueError):
        engine.predict_svm(np.zeros((3, 20)), model)
    small = cases.hand_model(2, 3)
    call_svm(engine, np.zeros((4, 2)), small, expect_error="nf = 65", nf=65)
    call_svm(engine, np.zeros((4, 2)), small, expect_error="nf = 0", nf=0)
    call_svm(engine, np.zeros((4, 2)), small, expect_error="n_sv = 0", n_sv=0)
    call_svm(engine, np.zeros((4, 2)), small._replace(gamma=0.0), expect_error="gamma")
    assert engine._lib.mrg_predict_svm(engine._h, 4, None, 2, None, None, None, None, 3, 0.0, 1.0, -1.0, 0.0, None, None, None,
                                       engine._stream_ptr()) == -1 and "null arrays" in error(engine)


# ------------------------------------------------------------------------------------------------ end to end
def read(path):
    with open(path) as fh:
        return fh.read()


def compare_with_rule(model, paths, table_text):
    """The five files against the rule run over the same table: filters and names as text, labels where the decision value
    is clear of 0, probabilities as numbers; the novel list's rows where no threshold is close.  Returns the rule's results."""
    want = rule.run(table_text, NAMELIST, model)
    for key in ("dataset", "refined_tmp", "refined"):
        assert read(paths[key]) == want[key]
    t = rule.tolerance(model)
    margin = cases.prob_margin(model, t)
    got, exp = read(paths["detailed"]).splitlines(), want["detailed"].splitlines()
    assert got[0] == exp[0] and len(got) == len(exp)
    for k, (a, b) in enumerate(zip(got[1:], exp[1:])):
        ca, cb = a.split(","), b.split(",")
        assert ca[2:] == cb[2:] and (ca[0] == cb[0] or abs(want["dec"][k]) <= t)
        assert abs(float(ca[1]) - float(cb[1])) <= margin and repr(float(ca[1])) == ca[1]
    if not cases.open_rows(model, want, t):
        strip = lambda text: [ln.split(",", 2)[2] for ln in text.splitlines()[1:]]
        assert strip(read(paths["novel"])) == strip(want["novel"])
    return want


@pytest.mark.parametrize("name", sorted(WORLDS))
def test_worlds_end_to_end_give_the_references_files(engine, model, tmp_path, name):
    from mirge_amd import predict
    world = WORLDS[name]
    text = cases.world_text(model, name)
    assert cases.text_digest(text) == world["sha256"]
    path = str(tmp_path / cases.TABLE)
    with open(path, "w") as fh:
        fh.write(text)
    models = cases.write_model_dir(str(tmp_path / "models"), model, "human")
    timings = {}
    got = predict.classify_candidates(engine, path, models, "human", timings=timings)
    assert set(timings) == {"read_s", "device_s", "write_s"}
    for key in ("dataset", "refined_tmp", "refined"):
        assert cases.text_digest(read(got["paths"][key])) == world["files"][key]          # byte for byte
    margin = cases.prob_margin(model, rule.tolerance(model))
    lines = read(got["paths"]["detailed"]).splitlines()
    assert lines[0] == "predictedValue,probability,realMicRNA,realMicRNAName,clusterName" and len(lines) - 1 == len(world["rows"])
    for ln, ref in zip(lines[1:], world["rows"]):
        c, r = ln.split(","), ref.split(",")
        assert c[0] == r[0] and abs(float(c[1]) - float(r[1])) <= margin and repr(float(c[1])) == c[1]
    novel = read(got["paths"]["novel"]).splitlines()
    assert novel[0] == lines[0] and [lines.index(ln) - 1 for ln in novel[1:]] == world["novel"]
    assert (got["table"], got["refined"], got["kept"]) == (text.count("\n") - 1, len(world["rows"]), len(world["novel"]))
    assert got["predicted"] == sum(r.startswith("1,") for r in world["rows"]) and got["stray"] == (1 if name == "stray" else 0)
    compare_with_rule(model, got["paths"], text)


def test_header_only_table_end_to_end(engine, model, tmp_path):
    from mirge_amd import predict
    path = str(tmp_path / cases.TABLE)
    with open(path, "w") as fh:
        fh.write(cases.header_only_text())
    got = predict.classify_candidates(engine, path, None, None, classifier=(model, NAMELIST))
    assert (got["table"], got["dataset"], got["refined"], got["predicted"], got["kept"]) == (0, 0, 0, 0, 0)
    assert all(read(p).count("\n") == 1 for p in got["paths"].values())


def test_map_and_cluster_and_the_shell_with_classify(engine, model, oracle_lib, tmp_path):
    from mirge_amd import predict
    from mirge_amd.index import FmIndex
    from tests import predict_screen_cases as screen_cases
    from tests.test_gpu_predict_precursors import synthetic_genome
    from tests.test_gpu_predict_trim import REPEATS_TSV
    names, texts, reads = synthetic_genome(np.random.default_rng(48))
    genome_prefix = str(tmp_path / "syn_genome")
    FmIndex.build(names, texts).save(genome_prefix + ".mrgfm")
    reads = list(dict.fromkeys(reads))
    fa = tmp_path / "unmapped_mirna_s1.fa"
    fa.write_text("".join(">mir%d_%d\n%s\n" % (k + 5, 4 + k % 5, r) for k, r in enumerate(reads)))
    (tmp_path / "rep.tsv").write_text(REPEATS_TSV)
    models = cases.write_model_dir(str(tmp_path / "models"), model, "others")
    shell = tmp_path / "shell"
    shell.mkdir()
    base = "unmapped_mirna_s1"
    cmd = str(tmp_path / "fold.sh")
    with open(cmd, "w") as fh:
        fh.write("#!/bin/sh\nexec '%s' '%s' \"$@\"\n" % (sys.executable, screen_cases.STANDIN))
    os.chmod(cmd, 0o755)
    common = ["clusters", genome_prefix, str(fa), "-o", str(shell / base), "--trim", "--repeats", str(tmp_path / "rep.tsv"), "-clc", "24",
              "--remap", "--features", "--precursors", "--screen", "--fold-cmd", cmd, "--classify"]
    # the model file is opened before any device work: nothing is written when it is missing or refused
    assert predict.main(common + ["--models", str(tmp_path / "nowhere"), "-sp", "zebrafish"]) == 1
    bad = cases.write_model_dir(str(tmp_path / "bad"), model, "others", kernel="linear")
    assert predict.main(common + ["--models", bad, "-sp", "zebrafish"]) == 1
    assert os.listdir(str(shell)) == []
    assert predict.main(common + ["--models", models, "-sp", "zebrafish"]) == 0
    screened = str(shell / (base + "_vs_representative_seq_modified_selected_sorted_features_updated_stableClusterSeq_15.tsv"))
    paths = predict.classified_paths(screened)
    assert os.path.basename(paths["novel"]) == "s1_novel_miRNAs_miRge2.0.csv" and all(os.path.exists(p) for p in paths.values())
    want = compare_with_rule(model, paths, read(screened))
    assert len(want["x"]) >= 1
    with pytest.raises(ValueError, match="classify needs screen"):
        predict.map_and_cluster(engine, str(fa), genome_prefix, 3, 25, 14, str(shell / "x"), classify=True, models=models, species="human")


def test_annotate_novel_predict_adds_the_files_per_sample(tmp_path_factory, native_lib, oracle_lib, model, tmp_path):
    from mirge_amd import cli, predict
    from mirge_amd.index import FmIndex
    from tests import predict_screen_cases as screen_cases
    from tests import util
    from tests.test_gpu_predict_precursors import synthetic_genome
    from tests.test_gpu_predict_trim import REPEATS_TSV
    w = util.World(n_fixed=600, n_var=150)
    root = str(tmp_path_factory.mktemp("model_libs") / "libs")
    w.libs.write_layout(root, species="syn", db="miRBase")
    rng = np.random.default_rng(47)
    names, texts, novel = synthetic_genome(rng)
    fastqs = []
    for i, name in enumerate(("left.fastq", "right.fastq")):
        reads = list(w.reads[i::2][:300]) + [r for r in novel for _ in range(int(rng.choice([3, 4, 5])))]
        fastqs.append(str(tmp_path / name))
        with open(fastqs[-1], "w") as fh:
            fh.write("".join("@r%d\n%s\n+\n%s\n" % (k, r, "I" * len(r)) for k, r in enumerate(reads)))
    FmIndex.build(names, texts).save(os.path.join(root, "syn", "index.Libs", "syn_genome") + ".mrgfm")
    os.makedirs(os.path.join(root, "syn", "annotation.Libs"), exist_ok=True)
    with open(os.path.join(root, "syn", "annotation.Libs", "syn_genome_repeats.tsv"), "w") as fh:
        fh.write(REPEATS_TSV)
    cmd = str(tmp_path / "fold.sh")
    with open(cmd, "w") as fh:
        fh.write("#!/bin/sh\nexec '%s' '%s' \"$@\"\n" % (sys.executable, screen_cases.STANDIN))
    os.chmod(cmd, 0o755)
    models = cases.write_model_dir(str(tmp_path / "models"), model, "others")
    args = ["annotate", "-s"] + fastqs + ["-lib", root, "-sp", "syn", "--novel-predict", "--fold-cmd", cmd, "-clc", "24", "-sl", "18"]
    with pytest.raises(SystemExit) as e:          # before any GPU work, as -pr is checked
        cli.annotate_main(cli.build_parser().parse_args(args + ["-o", str(tmp_path / "refused"), "--models", str(tmp_path / "nowhere")]))
    assert e.value.code == 1
    res = cli.annotate_main(cli.build_parser().parse_args(args + ["-o", str(tmp_path / "out"), "--models", models]))
    out = os.path.join(res["outdir"], "unmapped_tmp")
    for stem in ("left", "right"):
        sub = os.path.join(out, "unmapped_mirna_%s_tmp" % stem)
        screened = os.path.join(sub, "unmapped_mirna_%s_vs_representative_seq_modified_selected_sorted_features_updated_stableClusterSeq_15.tsv" % stem)
        paths = predict.classified_paths(screened)
        assert os.path.basename(paths["novel"]) == stem + "_novel_miRNAs_miRge2.0.csv"
        compare_with_rule(model, paths, read(screened))
