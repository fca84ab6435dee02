"""Predict mode's candidate reads on the GPU (-m gpu): mrg_predict_select, mrg_predict_sample_reads and mrg_predict_gather
against the plain-Python model (tests/predict_reads_model.py), field by field, and `annotate --novel-reads` /
`--novel-clusters` end to end: the FASTA files equal the model's over that run's own unmapped.csv, the cluster tables and
sorted SAM files equal predict.map_and_cluster's on the FASTA files the run wrote."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from tests import predict_reads_model as model

pytestmark = pytest.mark.gpu

MIN_LEN, MAX_LEN = 16, 25
SIZES = [0, 1, 63, 64, 65, 4097, 70001]
WIDTHS = [1, 2, 3, 33]          # sample columns: both sides of the switch to 16 lanes per row (16 columns)
BIG = 2 ** 32 - 1


@pytest.fixture(scope="module")
def engine(native_lib):
    from mirge_amd.engine import Engine
    eng = Engine(0)
    yield eng
    eng.close()


@functools.lru_cache(maxsize=None)
def world(n, S, mapped="mixed"):
    """(pass_id int8, lens uint8, quant uint32 [n, S]) and the model's answer for cutoff 2: lengths at the window's edges,
    small counts with zeros, and rows whose totals are 2^32 - 1, 2^32 and (three columns and more) 2^33."""
    rng = np.random.default_rng(1000 * S + n)
    lens = rng.choice([MIN_LEN - 1, MIN_LEN, 20, MAX_LEN, MAX_LEN + 1, 40, 255], size=n).astype(np.uint8)
    quant = rng.choice([0, 0, 0, 1, 1, 2, 3, 9], size=(n, S)).astype(np.uint32)
    pass_id = rng.choice(np.arange(-1, 9), size=n, p=[0.55] + [0.05] * 9).astype(np.int8)
    if mapped == "all":
        pass_id[:] = 3
    elif mapped == "none":
        pass_id[:] = -1
    if n >= 63:
        rows = [[BIG] + [0] * (S - 1)]
        if S >= 2:
            rows.append([BIG, 1] + [0] * (S - 2))
        if S >= 3:
            rows.append([BIG, BIG, 2] + [0] * (S - 3))
        for k, row in enumerate(rows):
            at = 7 + 11 * k
            quant[at], pass_id[at], lens[at] = row, (3 if mapped == "all" else -1), 20
    want = model.select(lens.tolist(), (pass_id < 0).tolist(), quant.tolist(), MIN_LEN, MAX_LEN, 2)
    return pass_id, lens, quant, want


def check_select(got, want, n):
    total, raw_no, sel_no, n_raw, n_sel = want
    assert (got["n_raw"], got["n_sel"]) == (n_raw, n_sel)
    assert got["total"].cpu().numpy().view(np.uint64).tolist() == total
    assert got["raw_no"].cpu().numpy().view(np.uint32).tolist() == raw_no
    assert got["sel_no"].cpu().numpy().view(np.uint32).tolist() == sel_no
    assert len(total) == n


@pytest.mark.parametrize("S", WIDTHS)
@pytest.mark.parametrize("n", SIZES)
def test_select_equals_the_model(engine, n, S):
    import torch
    pass_id, lens, quant, want = world(n, S)
    if n >= 63:
        assert BIG in want[0] and (S < 2 or 2 ** 32 in want[0]) and (S < 3 or 2 ** 33 in want[0])
        assert 0 < want[4] < want[3] < n
    check_select(engine.predict_select(pass_id, lens, quant, MIN_LEN, MAX_LEN, 2), want, n)       # host arrays
    if n <= 4097:                                                                                  # device tensors
        dev = engine.device
        d = (torch.from_numpy(pass_id.copy()).to(dev), torch.from_numpy(lens.copy()).to(dev),
             torch.from_numpy(quant.view(np.int32).copy()).to(dev))
        check_select(engine.predict_select(*d, MIN_LEN, MAX_LEN, 2), want, n)


@pytest.mark.parametrize("S", [2, 33])
def test_select_all_mapped_all_unmapped_and_the_cutoffs(engine, S):
    n = 4097
    pass_id, lens, quant, want = world(n, S, "all")
    assert want[3] == want[4] == 0 and not any(want[1])
    check_select(engine.predict_select(pass_id, lens, quant, MIN_LEN, MAX_LEN, 2), want, n)
    pass_id, lens, quant, want = world(n, S, "none")
    assert want[3] == sum(1 for t in want[0] if t >= 1)
    check_select(engine.predict_select(pass_id, lens, quant, MIN_LEN, MAX_LEN, 2), want, n)
    for cutoff in (1, 2 ** 40):          # every counted read in the window; above every total
        w = model.select(lens.tolist(), [True] * n, quant.tolist(), MIN_LEN, MAX_LEN, cutoff)
        assert (w[4] == 0) == (cutoff > 1) and w[3] == want[3]
        check_select(engine.predict_select(pass_id, lens, quant, MIN_LEN, MAX_LEN, cutoff), w, n)
    # a window of one length, and the lengths next to it
    for lo, hi in ((MIN_LEN, MIN_LEN), (MAX_LEN + 1, MAX_LEN + 1), (0, 255)):
        w = model.select(lens.tolist(), [True] * n, quant.tolist(), lo, hi, 2)
        assert w[4] > 0
        check_select(engine.predict_select(pass_id, lens, quant, lo, hi, 2), w, n)


@pytest.mark.parametrize("S", WIDTHS)
@pytest.mark.parametrize("n", SIZES)
def test_sample_reads_equal_the_model(engine, n, S):
    pass_id, lens, quant, want = world(n, S)
    sel = engine.predict_select(pass_id, lens, quant, MIN_LEN, MAX_LEN, 2)
    rows_q = quant.tolist()
    quant_d = engine._dev_u32(quant)
    for key, numbers, thr in (("raw_no", want[1], 1), ("sel_no", want[2], 2)):
        for s in range(S):
            got = engine.predict_sample_reads(quant_d, sel[key], s, thr)
            got = [t.cpu().numpy().view(np.uint32).tolist() for t in got]
            exp = model.sample_rows(numbers, rows_q, s, thr)
            assert got == [[r[k] for r in exp] for k in range(3)], (key, s)
    if n:   # host arrays as input
        got = engine.predict_sample_reads(quant, np.array(want[2], np.uint32), 0, 2)
        exp = model.sample_rows(want[2], rows_q, 0, 2)
        assert [t.cpu().numpy().view(np.uint32).tolist() for t in got] == [[r[k] for r in exp] for k in range(3)]


def test_a_sample_without_rows_and_the_read_only_the_sum_admits(engine):
    rng = np.random.default_rng(9)
    n, S = 300, 3
    lens = np.full(n, 20, np.uint8)
    pass_id = np.full(n, -1, np.int8)
    quant = rng.choice([0, 1, 2, 5], size=(n, S)).astype(np.uint32)
    quant[:, 1] = 0                         # a sample no read has a count in
    quant[17] = [1, 0, 1]                   # below the cutoff in every sample, the sum reaches it
    sel = engine.predict_select(pass_id, lens, quant, MIN_LEN, MAX_LEN, 2)
    want = model.select(lens.tolist(), [True] * n, quant.tolist(), MIN_LEN, MAX_LEN, 2)
    check_select(sel, want, n)
    assert want[2][17] > 0
    for key, thr in (("raw_no", 1), ("sel_no", 2)):
        idx, num, cnt = engine.predict_sample_reads(quant, sel[key], 1, thr)
        assert idx.numel() == num.numel() == cnt.numel() == 0
    for s in (0, 2):
        idx, _, _ = engine.predict_sample_reads(quant, sel["sel_no"], s, 2)
        assert idx.numel() > 0 and 17 not in idx.cpu().tolist()
        idx, _, cnt = engine.predict_sample_reads(quant, sel["raw_no"], s, 1)
        assert 17 in idx.cpu().tolist()


@pytest.mark.parametrize("with_n", [False, True])
@pytest.mark.parametrize("W", [1, 2, 8])
def test_gather_equals_the_models_sequences(engine, W, with_n):
    from mirge_amd import pack
    rng = np.random.default_rng(10 * W + with_n)
    hi = {1: 32, 2: 64, 8: 255}[W]
    seqs = model.random_reads(rng, 700, [15, 16, 20, 25, 26, hi - 1, hi], p_n=0.04 if with_n else 0.0)
    words, lens, nmask = pack.pack_reads(seqs, W)
    assert words.shape[0] == W and (nmask is not None) == with_n
    quant = rng.choice([0, 1, 2, 7], size=(len(seqs), 2)).astype(np.uint32)
    pass_id = rng.choice([-1, -1, 4], size=len(seqs)).astype(np.int8)
    sel = engine.predict_select(pass_id, lens, quant, MIN_LEN, hi, 2)
    want = model.select(lens.tolist(), (pass_id < 0).tolist(), quant.tolist(), MIN_LEN, hi, 2)
    for s in (0, 1, None):
        if s is None:
            exp = [(u, no, want[0][u]) for u, no in enumerate(want[2]) if no]
            idx = np.array([r[0] for r in exp], np.uint32)
        else:
            exp = model.sample_rows(want[2], quant.tolist(), s, 2)
            idx = engine.predict_sample_reads(quant, sel["sel_no"], s, 2)[0]
        g_words, g_lens, g_nmask, g_counts = engine.predict_gather(words, lens, nmask, quant, idx, sample=s)
        assert tuple(g_words.shape) == (W, len(exp)) and (g_nmask is not None) == with_n and len(exp) > 50
        got = pack.unpack_reads(g_words.cpu().numpy().view(np.uint64), g_lens.cpu().numpy(),
                                None if g_nmask is None else g_nmask.cpu().numpy().view(np.uint64))
        assert got == [seqs[r[0]] for r in exp]
        assert g_counts.cpu().numpy().view(np.uint32).tolist() == [r[2] for r in exp]
        assert any(len(q) == hi for q in got)
    # no row
    out = engine.predict_gather(words, lens, nmask, quant, np.zeros(0, np.uint32), sample=0)
    assert out[0].shape[1] == 0 and out[3].numel() == 0


def test_gather_refuses_what_it_cannot_deliver(engine):
    from mirge_amd import pack
    from mirge_amd._native import MirgeAmdError
    seqs = ["ACGTACGTACGTACGTAC", "TTTTACGTACGTACGTACGT", "GGGGACGTACGTACGTACA"]
    words, lens, nmask = pack.pack_reads(seqs)
    quant = np.array([[BIG, 1], [3, 4], [BIG, 0]], np.uint32)
    with pytest.raises(MirgeAmdError, match="no read"):
        engine.predict_gather(words, lens, nmask, quant, np.array([0, 3], np.uint32), sample=0)
    with pytest.raises(MirgeAmdError, match="32 bits"):
        engine.predict_gather(words, lens, nmask, quant, np.array([0, 1], np.uint32))
    with pytest.raises(MirgeAmdError, match="sample 2 of 2"):
        engine.predict_gather(words, lens, nmask, quant, np.array([0, 1], np.uint32), sample=2)
    out = engine.predict_gather(words, lens, nmask, quant, np.array([1, 2], np.uint32))
    assert out[3].cpu().numpy().view(np.uint32).tolist() == [7, BIG]
    with pytest.raises(MirgeAmdError, match="window"):
        engine.predict_select(np.zeros(3, np.int8), lens, quant, 26, 25, 2)
    with pytest.raises(MirgeAmdError, match="cutoff"):
        engine.predict_select(np.zeros(3, np.int8), lens, quant, 16, 25, 0)
    # device tensors of another element type are refused, not read with the wrong element size
    import torch
    dev = engine.device
    d_pass, d_lens = torch.zeros(3, dtype=torch.int8, device=dev), torch.from_numpy(lens.copy()).to(dev)
    d_quant = torch.from_numpy(quant.view(np.int32).copy()).to(dev)
    assert engine.predict_select(d_pass, d_lens, d_quant, 16, 25, 2)["n_raw"] == 0
    with pytest.raises(TypeError, match="pass_id"):
        engine.predict_select(d_pass.to(torch.int32), d_lens, d_quant, 16, 25, 2)
    with pytest.raises(TypeError, match="lens"):
        engine.predict_select(d_pass, d_lens.to(torch.int8), d_quant, 16, 25, 2)
    with pytest.raises(TypeError, match="quant"):
        engine.predict_select(d_pass, d_lens, d_quant.to(torch.int64), 16, 25, 2)
    with pytest.raises(TypeError, match="numbers"):
        engine.predict_sample_reads(d_quant, torch.ones(3, dtype=torch.int64, device=dev), 0, 1)
    with pytest.raises(TypeError, match="index"):
        engine.predict_gather(words, lens, nmask, d_quant, torch.zeros(2, dtype=torch.int64, device=dev), sample=0)
    rows = C.c_uint64()
    tmp = engine._predict_tmp(3)
    q, no = engine._dev_u32(quant), engine._dev_u32(np.array([1, 2, 3], np.uint32))
    out = engine._dev_u32(np.full(3, 0xFFFFFFFF, np.uint32))
    L = engine._lib
    # a buffer smaller than the rows: the count comes back, no row is written
    assert L.mrg_predict_sample_reads(engine._h, q.data_ptr(), 3, 2, 0, no.data_ptr(), 1, out.data_ptr(), out.data_ptr(),
                                      out.data_ptr(), 1, C.byref(rows), tmp.data_ptr(), tmp.numel(), engine._stream_ptr()) < 0
    assert b"do not fit" in L.mrg_last_error() and rows.value == 3 and out.cpu().tolist() == [-1, -1, -1]
    assert L.mrg_predict_sample_reads(engine._h, q.data_ptr(), 3, 2, 1, no.data_ptr(), 1, None, None, None, 0, C.byref(rows),
                                      tmp.data_ptr(), tmp.numel(), engine._stream_ptr()) < 0 and rows.value == 2
    assert L.mrg_predict_sample_reads(engine._h, q.data_ptr(), 3, 2, 1, no.data_ptr(), 5, None, None, None, 0, C.byref(rows),
                                      tmp.data_ptr(), tmp.numel(), engine._stream_ptr()) == 0 and rows.value == 0
    assert L.mrg_predict_sample_reads(engine._h, q.data_ptr(), 3, 2, 0, no.data_ptr(), 1, out.data_ptr(), out.data_ptr(),
                                      out.data_ptr(), 3, C.byref(rows), tmp.data_ptr(), 16, engine._stream_ptr()) < 0
    assert b"scratch" in L.mrg_last_error()


# ------------------------------------------------------------------------------------------------------- command line
def rand_seq(rng, L):
    return "".join("ACGT"[c] for c in rng.integers(0, 4, L))


def write_fastqs(tmp_path, samples):
    paths = []
    for name, reads in samples:
        paths.append(str(tmp_path / name))
        with open(paths[-1], "w") as fh:
            fh.write("".join("@r%d\n%s\n+\n%s\n" % (k, r, "I" * len(r)) for k, r in enumerate(reads)))
    return paths


@pytest.fixture(scope="module")
def small_world(tmp_path_factory, native_lib):
    from tests import util
    w = util.World(n_fixed=600, n_var=150)
    root = str(tmp_path_factory.mktemp("novel_libs") / "libs")
    w.libs.write_layout(root, species="syn", db="miRBase")
    return w, root


def annotate(fastqs, root, out, *extra):
    from mirge_amd import cli
    res = cli.annotate_main(cli.build_parser().parse_args(
        ["annotate", "-s"] + fastqs + ["-lib", root, "-sp", "syn", "-o", str(out)] + list(extra)))
    return res["outdir"]


def test_cli_novel_reads_equals_the_model_over_its_own_unmapped_csv(small_world, tmp_path):
    w, root = small_world
    rng = np.random.default_rng(31)
    long_read = rand_seq(rng, 263)
    novel = [rand_seq(rng, int(L)) for L in rng.choice([15, 16, 17, 22, 25, 26, 30], 120)]
    novel[0] = rand_seq(rng, 20)
    novel += [s[:4] + "N" + s[5:] for s in novel[:10]]
    samples = []
    for i, name in enumerate(("left.fastq", "right.fastq")):
        reads = list(w.reads[i::2])
        reads += [r for r in novel[1:] for _ in range(int(rng.choice([0, 1, 1, 2, 3, 6])))]
        reads += [novel[0]] + [long_read] * (1 + i)          # novel[0]: one copy each -- the sum reaches 2, no sample does
        samples.append((name, reads))
    fastqs = write_fastqs(tmp_path, samples)
    out = annotate(fastqs, root, tmp_path / "out", "--novel-reads")
    got_dir = os.path.join(out, "unmapped_tmp")
    got = {fn: open(os.path.join(got_dir, fn)).read() for fn in sorted(os.listdir(got_dir))}
    names, seqs, quant = model.from_csv(open(os.path.join(out, "unmapped.csv")).read())
    assert names == ["left.fastq", "right.fastq"]
    want = model.files(names, seqs, quant, 16, 25, 2)
    assert sorted(got) == sorted(want) == sorted(["unmapped_mirna.fa", "unmapped_mirna_raw.fa", "unmapped_mirna_left.fa",
                                                  "unmapped_mirna_left_raw.fa", "unmapped_mirna_right.fa",
                                                  "unmapped_mirna_right_raw.fa"])
    assert got == want
    assert seqs[-1] == long_read and quant[-1] == [1, 2]
    n_raw = got["unmapped_mirna_raw.fa"].count(">")
    assert got["unmapped_mirna_raw.fa"].endswith(">mir%d_3\n%s\n" % (n_raw, long_read)) and n_raw > 100
    assert got["unmapped_mirna_right_raw.fa"].endswith(">mir%d_2\n%s\n" % (n_raw, long_read))
    assert long_read not in got["unmapped_mirna.fa"] and got["unmapped_mirna.fa"].count(">") > 20
    assert novel[0] in got["unmapped_mirna.fa"] and novel[0] not in got["unmapped_mirna_left.fa"] + got["unmapped_mirna_right.fa"]
    assert "N" in got["unmapped_mirna_raw.fa"]
    # a wider window admits the long read into the filtered files too
    out = annotate(fastqs, root, tmp_path / "wide", "--novel-reads", "-maxl", "300", "-cc", "1")
    got_dir = os.path.join(out, "unmapped_tmp")
    got = {fn: open(os.path.join(got_dir, fn)).read() for fn in sorted(os.listdir(got_dir))}
    names, seqs, quant = model.from_csv(open(os.path.join(out, "unmapped.csv")).read())
    assert got == model.files(names, seqs, quant, 16, 300, 1) and long_read in got["unmapped_mirna_left.fa"]


def test_cli_novel_clusters_equals_map_and_cluster_on_its_own_fasta(small_world, engine, tmp_path, capsys):
    from mirge_amd import predict
    from mirge_amd.index import FmIndex
    import shutil
    w, root0 = small_world
    root = str(tmp_path / "libs")
    shutil.copytree(root0, root)
    rng = np.random.default_rng(47)
    names = ["chr1", "chr2", "scaffold_9"]
    texts = [rand_seq(rng, 20000) for _ in names]
    comp = str.maketrans("ACGT", "TGCA")
    novel = []
    for _ in range(400):   # piles around a few loci, both strands
        e = int(rng.integers(0, 3))
        at = int(rng.choice([500, 530, 4000, 4010, 9000])) + int(rng.integers(-12, 13))
        q = texts[e][at:at + int(rng.integers(16, 27))]
        novel.append(q[::-1].translate(comp) if rng.random() < 0.4 else q)
    novel = list(dict.fromkeys(novel))
    samples = []
    for i, name in enumerate(("left.fastq", "right.fastq")):
        reads = list(w.reads[i::2][:300])
        reads += [r for r in novel for _ in range(int(rng.choice([0, 1, 2, 3, 5])))]
        samples.append((name, reads))
    fastqs = write_fastqs(tmp_path, samples)
    # no genome next to the libraries: -ai's message, exit status 1, nothing written
    with pytest.raises(SystemExit) as ei:
        annotate(fastqs, root, tmp_path / "nogenome", "--novel-clusters")
    assert ei.value.code == 1 and "syn_genome" in capsys.readouterr().out and not os.path.exists(str(tmp_path / "nogenome"))
    genome = os.path.join(root, "syn", "index.Libs", "syn_genome")
    FmIndex.build(names, texts).save(genome + ".mrgfm")
    with pytest.raises(SystemExit) as ei:
        annotate(fastqs, root, tmp_path / "toolong", "--novel-clusters", "-maxl", "300")
    assert ei.value.code == 1 and "255" in capsys.readouterr().err and not os.path.exists(str(tmp_path / "toolong"))
    out = annotate(fastqs, root, tmp_path / "out", "--novel-clusters")
    top = os.path.join(out, "unmapped_tmp")
    assert sorted(os.listdir(top)) == ["unmapped_mirna.fa", "unmapped_mirna_left_tmp", "unmapped_mirna_raw.fa",
                                       "unmapped_mirna_right_tmp"]
    csv = model.from_csv(open(os.path.join(out, "unmapped.csv")).read())
    want = model.files(csv[0], csv[1], csv[2], 16, 25, 2)
    for stem in ("left", "right"):
        sub = os.path.join(top, "unmapped_mirna_%s_tmp" % stem)
        base = "unmapped_mirna_" + stem
        assert sorted(os.listdir(sub)) == [base + ".fa", base + "_raw.fa", base + "_vs_genome_sorted.sam",
                                           base + "_vs_genome_sorted_clusters.tsv"]
        for fn in (base + ".fa", base + "_raw.fa"):
            assert open(os.path.join(sub, fn)).read() == want[fn]
        ref = tmp_path / ("ref_" + stem)
        ref.mkdir()
        cl = predict.map_and_cluster(engine, os.path.join(sub, base + ".fa"), genome, 3, 25, 14, str(ref / base))
        assert len(cl["entry"]) > 3 and cl["n_rows"] > 30
        for fn in (base + "_vs_genome_sorted.sam", base + "_vs_genome_sorted_clusters.tsv"):
            assert open(os.path.join(sub, fn), "rb").read() == (ref / fn).read_bytes(), fn
    for fn in ("unmapped_mirna.fa", "unmapped_mirna_raw.fa"):
        assert open(os.path.join(top, fn)).read() == want[fn]
    # without the flags: no directory
    plain = annotate(fastqs, root, tmp_path / "plain")
    assert not os.path.exists(os.path.join(plain, "unmapped_tmp")) and os.path.exists(os.path.join(plain, "unmapped.csv"))
