"""Predict mode's report on the GPU: each device call (mrg_predict_report_correct / _entries / _profile) on device buffers with
guard words behind every output, against tests/predict_report_model.py, in the smallest shapes that can go wrong; then the
fixture's worlds end to end through predict.report_candidates, byte-equal to the reference's two files and to the rows the
reference handed to its drawing; the raising cases; a precursor of 257 characters on the host path; and the two shells."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from tests import predict_report_cases as cases
from tests import predict_report_model as rule
from tests.test_predict_report_native import check_against_fixture, read, write_inputs

pytestmark = pytest.mark.gpu
GUARD = 8


@pytest.fixture(scope="module")
def engine(native_lib):
    from mirge_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


class Guarded:
    """Device outputs with GUARD words of a pattern behind each; check() says none was written."""

    def __init__(self, engine):
        import torch
        self.torch, self.engine, self.made = torch, engine, []

    def __call__(self, count, dtype):
        t = self.torch.full((int(count) + GUARD,), 0x5a, dtype=dtype, device=self.engine.device)
        self.made.append((t, int(count)))
        return t

    def check(self):
        for t, count in self.made:
            assert bool((t[count:] == 0x5a).all()), "a guard word behind an output of %d was written" % count


def device_run(engine, texts):
    """The three calls over the rule's arrays for `texts`, every output guarded; returns host arrays cut to their sizes."""
    import torch
    from mirge_amd._native import check
    lib, p, st = engine._lib, engine._p, engine._stream_ptr
    want = rule.run(*texts)
    d = engine.predict_report_upload(rule.arrays(*texts))
    n = d["n"]
    g = Guarded(engine)
    lines = dict(src=g(n, torch.int32), state=g(n, torch.uint8), err=g(n, torch.uint8), pos_adj=g(2 * n, torch.int64),
                 stable_idx=g(n, torch.int32), gid=g(n, torch.int32))
    check(lib.mrg_predict_report_correct(engine._h, n, p(d["flags"]), p(d["up"]), p(d["down"]), p(d["pos"]), p(d["adj"]), p(d["gid3"]),
                                         p(d["t_off"]), p(d["text"]), int(d["text"].numel()), p(lines["src"]), p(lines["state"]),
                                         p(lines["err"]), p(lines["pos_adj"]), p(lines["stable_idx"]), p(lines["gid"]), st()))
    g.check()
    got = {k: lines[k][:n * (2 if k == "pos_adj" else 1)].cpu().numpy() for k in lines}
    assert not got["err"].any()
    assert np.array_equal(got["src"].view(np.uint32), want["src"])
    assert np.array_equal(got["pos_adj"].reshape(n, 2), want["pos_adj"])
    host = (want["state"] & 4) != 0
    assert np.array_equal((got["state"] & 4) != 0, host)
    assert np.array_equal(got["state"][~host], want["state"][~host])
    assert np.array_equal(got["stable_idx"][~host], want["stable_idx"][~host])
    assert np.array_equal(got["state"][host] & 0x0d, want["state"][host] & 0x0d)   # touched, host, none: known without the strings
    if host.any():   # the caller's part: re-type and stable index of the lines left to the host
        lines["state"][:n] = torch.from_numpy(want["state"]).to(engine.device)
        lines["stable_idx"][:n] = torch.from_numpy(want["stable_idx"]).to(engine.device)
    # groups: equal ids exactly where (corrected precursor, chr, strand) are equal, none where the precursor is None
    gid = got["gid"].view(np.uint32)
    assert np.array_equal(gid == rule.NO_GROUP, (want["state"] & 8) != 0)
    ents = dict(ent_m=g(n, torch.int32), ent_p=g(n, torch.int32), chunk_err=g(n, torch.uint8), chunk_line=g(n, torch.int32),
                row_off=g(n + 1, torch.int64), prof_off=g(n + 1, torch.int64))
    totals = (C.c_uint64 * 3)()
    tmp = engine._report_tmp(n)
    check(lib.mrg_predict_report_entries(engine._h, n, p(d["flags"]), p(d["rank"]), p(d["reads"]), p(d["t_off"]), p(lines["src"]),
                                         p(lines["state"]), p(lines["stable_idx"]), p(lines["gid"]), p(d["blk"]), p(d["r_off"]),
                                         p(ents["ent_m"]), p(ents["ent_p"]), p(ents["chunk_err"]), p(ents["chunk_line"]), p(ents["row_off"]),
                                         p(ents["prof_off"]), totals, tmp.data_ptr(), tmp.numel(), st()))
    g.check()
    E = int(totals[0])
    assert E == want["n_entries"] and int(totals[1]) == len(want["lead"]) and int(totals[2]) == len(want["prof"])
    assert not ents["chunk_err"][:n].cpu().numpy().any()
    assert np.array_equal(ents["ent_m"][:E].cpu().numpy().view(np.uint32), want["ent_m"])
    assert np.array_equal(ents["ent_p"][:E].cpu().numpy(), want["ent_p"])
    assert np.array_equal(ents["row_off"][:E + 1].cpu().numpy().view(np.uint64), want["row_off"])
    assert np.array_equal(ents["prof_off"][:E + 1].cpu().numpy().view(np.uint64), want["prof_off"])
    chunk_lines = ents["chunk_line"][:len(want["chunks"])].cpu().numpy().view(np.uint32)
    assert chunk_lines.tolist() == [m for m, _ in want["chunks"]]
    R, W = len(want["lead"]), len(want["prof"])
    prof = dict(lead=g(R, torch.int32), trail=g(R, torch.int32), prof=g(W, torch.int64), total=g(E, torch.int64), flag=g(E, torch.uint8))
    check(lib.mrg_predict_report_profile(engine._h, n, p(d["flags"]), p(d["t_off"]), p(d["text"]), int(d["text"].numel()), p(lines["src"]),
                                         p(lines["pos_adj"]), p(lines["stable_idx"]), p(d["r_off"]), d["n_rows"], p(d["row_start"]),
                                         p(d["row_end"]), p(d["row_count"]), p(d["row_soff"]), p(d["row_text"]), int(d["row_text"].numel()), E,
                                         p(ents["ent_m"]), p(ents["ent_p"]), p(ents["row_off"]), p(ents["prof_off"]), p(prof["lead"]),
                                         p(prof["trail"]), p(prof["prof"]), p(prof["total"]), p(prof["flag"]), st()))
    g.check()
    flag = prof["flag"][:E].cpu().numpy()
    assert np.array_equal((flag & 2) != 0, (want["flag"] & 2) != 0) and not (flag & 4).any()
    for e in np.flatnonzero((flag & 2) == 0).tolist():
        r0, r1, p0, p1 = (int(v) for v in (want["row_off"][e], want["row_off"][e + 1], want["prof_off"][e], want["prof_off"][e + 1]))
        assert np.array_equal(prof["lead"][r0:r1].cpu().numpy(), want["lead"][r0:r1])
        assert np.array_equal(prof["trail"][r0:r1].cpu().numpy(), want["trail"][r0:r1])
        assert np.array_equal(prof["prof"][p0:p1].cpu().numpy().view(np.uint64), want["prof"][p0:p1])
        assert int(prof["total"][e].cpu().numpy().view(np.uint64)) == int(want["total"][e]) and flag[e] == want["flag"][e]
    return want


@pytest.mark.parametrize("n_lines", [1, 2, 63, 64, 65])
def test_tables_of_every_size_around_a_wave(engine, n_lines):
    want = device_run(engine, cases.shape_world(n_lines, 80, "first"))
    assert want["n_entries"] == n_lines


@pytest.mark.parametrize("prec_len", [1, 63, 64, 65, 255, 256])
def test_precursor_lengths_and_cluster_placements(engine, prec_len):
    for placement in ("first", "last", "middle", "straddle", "absent", "longer"):
        want = device_run(engine, cases.shape_world(3, prec_len, placement))
        if prec_len < 255 or placement != "longer":
            assert not (want["state"] & 4).any()           # inside the kernels' limits: nothing is left to the host
    assert (device_run(engine, cases.shape_world(3, 130, "middle"))["state"] & 2).any()   # one of them is re-typed


@pytest.mark.parametrize("n_rows", [1, 63, 64, 65, 130])
def test_read_rows_around_the_tile(engine, n_rows):
    want = device_run(engine, cases.shape_world(2, 70, "first", n_rows=n_rows))
    assert want["n_entries"] == 2 and len(want["lead"]) == 2 * n_rows


def test_sums_beyond_32_bits(engine):
    want = device_run(engine, cases.shape_world(2, 70, "first", n_rows=3, count=3_000_000_000))
    assert int(want["prof"].max()) > 2 ** 32 and int(want["total"].max()) > 2 ** 33


def test_zero_entries_and_zero_lines(engine, tmp_path):
    from mirge_amd import predict
    device_run(engine, cases.world("nothing_listed"))
    header_only = (cases.NOVEL_HEADER, "\t".join(cases.HEADER) + "\n", "")
    device_run(engine, header_only)
    got = predict.report_candidates(engine, dict(zip(("novel", "table", "cluster"), write_inputs(tmp_path, header_only))))
    assert got["entries"] == 0 and read(got["paths"]["report"]) == rule.REPORT_HEADER and read(got["paths"]["profiles"]) == ""
    assert read(got["paths"]["corrected"]) == header_only[1]


@pytest.mark.parametrize("name", cases.WORLDS)
def test_worlds_end_to_end(engine, name, tmp_path):
    from mirge_amd import predict
    texts = cases.world(name)
    device_run(engine, texts)
    novel, table, _ = write_inputs(tmp_path, texts)
    timings = {}
    got = predict.report_candidates(engine, dict(paths=dict(novel=novel), screened=table), threads=2, timings=timings)   # a classify result's form
    assert set(timings) == {"read_s", "device_s", "write_s"} and got["host_lines"] == 0 and got["host_entries"] == 0
    files = {key: read(got["paths"][key]) for key in ("corrected", "report", "profiles")}
    check_against_fixture(name, texts, files)
    want = rule.run(*texts)
    assert files["profiles"] == want["profiles"] and got["entries"] == want["n_entries"] == files["report"].count("\n") - 1


@pytest.mark.parametrize("name", sorted(cases.raising_cases()))
def test_raising_cases_raise_and_write_nothing(engine, name, tmp_path):
    from mirge_amd import predict
    paths = write_inputs(tmp_path, cases.raising_cases()[name])
    with pytest.raises(ValueError, match="line [0-9]+ of the table"):
        predict.report_candidates(engine, dict(zip(("novel", "table", "cluster"), paths)))
    assert sorted(os.listdir(str(tmp_path))) == sorted(os.path.basename(p) for p in paths)


def test_a_precursor_of_257_characters_takes_the_host_path(engine, tmp_path):
    from mirge_amd import predict
    a, b, c = cases.shape_world(3, 80, "first"), cases.shape_world(1, 257, "middle", seed=5), cases.shape_world(2, 256, "last", seed=6)
    renumber = lambda text, k: text.replace("miRCluster_", "miRCluster_%d" % k)
    texts = (a[0] + "".join(renumber(t[0], k).split("\n", 1)[1] for k, t in ((7, b), (8, c))),
             a[1] + "".join(renumber(t[1], k).split("\n", 1)[1] for k, t in ((7, b), (8, c))),
             a[2] + renumber(b[2], 7) + renumber(c[2], 8))
    want = rule.run(*texts)
    assert want["host_lines"] == 1 and int(((want["flag"] & 2) != 0).sum()) == 1 and want["n_entries"] == 6
    device_run(engine, texts)
    got = predict.report_candidates(engine, dict(zip(("novel", "table", "cluster"), write_inputs(tmp_path, texts))))
    assert got["host_lines"] == 1 and got["host_entries"] == 1
    for key in ("corrected", "report", "profiles"):
        assert read(got["paths"][key]) == want[key], key


def compare_with_rule(novel, table):
    from mirge_amd import predict
    cluster = predict._report_cluster_path(table)
    paths = predict.report_paths(novel, table, cluster)
    want = rule.run(read(novel), read(table), read(cluster))
    for key in ("corrected", "report", "profiles"):
        assert read(paths[key]) == want[key], key
    return paths, want


def test_the_shell_with_report(engine, oracle_lib, tmp_path):
    from mirge_amd import predict
    from mirge_amd.index import FmIndex
    from tests import predict_model_cases as model_cases
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
    models = model_cases.write_model_dir(str(tmp_path / "models"), model_cases.fixture_model(), "others")
    shell = tmp_path / "shell"
    shell.mkdir()
    base = "unmapped_mirna_s1"
    cmd = str(tmp_path / "fold.sh")
    with open(cmd, "w") as fh:
        fh.write("#!/bin/sh\nexec '%s' '%s' \"$@\"\n" % (sys.executable, screen_cases.STANDIN))
    os.chmod(cmd, 0o755)
    common = ["clusters", genome_prefix, str(fa), "-o", str(shell / base), "--trim", "--repeats", str(tmp_path / "rep.tsv"), "-clc", "24",
              "--remap", "--features", "--precursors", "--screen", "--fold-cmd", cmd]
    with pytest.raises(SystemExit):
        predict.main(common + ["--report"])          # --report needs --classify
    assert predict.main(common + ["--classify", "--models", models, "-sp", "zebrafish", "--report"]) == 0
    screened = str(shell / (base + "_vs_representative_seq_modified_selected_sorted_features_updated_stableClusterSeq_15.tsv"))
    paths, _ = compare_with_rule(predict.classified_paths(screened)["novel"], screened)
    assert os.path.basename(paths["report"]) == "s1_novel_miRNAs_report.csv"
    with pytest.raises(ValueError, match="report needs classify"):
        predict.map_and_cluster(engine, str(fa), genome_prefix, 3, 25, 14, str(shell / "x"), report=True)


def test_annotate_novel_report_adds_the_files_and_the_directory(tmp_path_factory, native_lib, oracle_lib, tmp_path):
    from mirge_amd import cli, predict
    from mirge_amd.index import FmIndex
    from tests import predict_model_cases as model_cases
    from tests import predict_screen_cases as screen_cases
    from tests import util
    from tests.test_gpu_predict_precursors import synthetic_genome
    from tests.test_gpu_predict_trim import REPEATS_TSV
    w = util.World(n_fixed=600, n_var=150)
    root = str(tmp_path_factory.mktemp("report_libs") / "libs")
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
    models = model_cases.write_model_dir(str(tmp_path / "models"), model_cases.fixture_model(), "others")
    args = ["annotate", "-s"] + fastqs + ["-lib", root, "-sp", "syn", "--novel-report", "--fold-cmd", cmd, "-clc", "24", "-sl", "18"]
    res = cli.annotate_main(cli.build_parser().parse_args(args + ["-o", str(tmp_path / "out"), "--models", models]))
    out = os.path.join(res["outdir"], "unmapped_tmp")
    for stem in ("left", "right"):
        sub = os.path.join(out, "unmapped_mirna_%s_tmp" % stem)
        screened = os.path.join(sub, "unmapped_mirna_%s_vs_representative_seq_modified_selected_sorted_features_updated_stableClusterSeq_15.tsv" % stem)
        paths, want = compare_with_rule(predict.classified_paths(screened)["novel"], screened)
        novel_dir = os.path.join(res["outdir"], stem + "_novel_miRNAs")
        assert sorted(os.listdir(novel_dir)) == [stem + "_novel_miRNAs_report.csv", stem + "_novel_miRNAs_report_profiles.tsv"]
        assert read(os.path.join(novel_dir, stem + "_novel_miRNAs_report.csv")) == want["report"]
        assert read(os.path.join(novel_dir, stem + "_novel_miRNAs_report_profiles.tsv")) == want["profiles"]
