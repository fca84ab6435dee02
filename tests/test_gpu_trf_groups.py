"""The array route of tRFs.samples.tmp/ on the GPU: Engine.trf_sample_groups (csrc/trf_groups.hip through
mrg_trf_sample_groups) field by field against the numpy statement (tests/trf_groups_model.py), TrfPeaks.rank()
(mrg_trf_rank) against the per-group stable argsort, Engine.trf_peaks_groups against Engine.trf_peaks on the downloaded
layout, and `annotate -trf` end to end with the per-read Python of the record route made to raise."""
import ctypes as C
import os
import types

import numpy as np
import pytest

from mirge_amd import trf, trf_samples
from tests.test_trf_groups import arrays_of, golden_arrays, hand_world, rand_seq
from tests.test_trf_samples import WORLDS, check_dir, golden  # noqa: F401  (golden: the module fixture)
from tests.trf_groups_model import model_groups
from tests.trf_peaks_model import random_rows

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine(native_lib):
    from mirge_amd.engine import Engine
    return Engine(0)


def assert_equal_to_model(engine, a, timings=None):
    want = model_groups(a.st, a.rec, a.words, a.lens, a.nmask, a.quant, a.denom)
    got = engine.trf_sample_groups(a.st, a.rec, a.words, a.lens, a.nmask, a.quant, a.denom, timings=timings)
    for f in ("n_items", "G", "n", "max_len", "has_n", "no_template_row", "filled"):
        assert getattr(got, f) == getattr(want, f), f
    if not want.filled:
        return got, want
    for f in ("blocks", "block_sums", "off", "groups", "rows", "codes", "span"):
        assert np.array_equal(getattr(got, f), getattr(want, f)), f
    assert (got.nmask is None) == (want.nmask is None) and (want.nmask is None or np.array_equal(got.nmask, want.nmask))
    assert np.array_equal(got.rpm.view(np.uint64), want.rpm.view(np.uint64))
    return got, want


def random_world(seed, n_rows, S, n_trna, read_len, tmpl_len, with_n, exact_items=False, spare=7):
    """n_rows tsv rows over n_trna mature and a few trailer templates, reads of read_len = (lo, hi) nt: every 5th read
    is a variant of the one before (a proper prefix, another last base, an N, one base more) on the same tRNA and start
    with the same counts; starts run up to 3 nt past the last one that fits; rows of kind 5 and reads that no row names
    lie in between.  exact_items: every classified row has a count in exactly one sample."""
    rng = np.random.default_rng(seed)
    names = ["t%02d" % i for i in range(n_trna)] + ["pre_t%02d_trailer" % i for i in range(3)] + ["t01"]
    tmpl = {n: rand_seq(rng, int(rng.integers(tmpl_len[0], tmpl_len[1] + 1))) for n in names}
    tables = {"trnaStruDic": {k: {"seq": v} for k, v in tmpl.items() if "pre" not in k},
              "trnaAAanticodonDic": {k: {"aaType": "A%d" % (i % 9), "anticodon": "XXX"} for i, k in enumerate(names)}}
    pre = {k: v for k, v in tmpl.items() if "pre" in k}
    reads, quant, rows, seen = [], [], [], set()
    prev = None
    while len(rows) < n_rows:
        if len(reads) % spare == 3:                                      # a read of another pass
            reads.append(rand_seq(rng, int(rng.integers(12, 24))) + "CCCC")
            quant.append(rng.integers(0, 9, S).tolist())
            continue
        if prev is not None and len(rows) % 5 == 4:
            read, entry, start, counts = prev
            read = (read[:-1], read[:-1] + "ACGTN"[int(rng.integers(0, 5))], read + "A", read[:-2] + "N" + read[-1])[len(rows) % 4]
            if not with_n:
                read = read.replace("N", "G")
        else:
            entry = int(rng.integers(0, len(names)))
            L = int(rng.integers(read_len[0], read_len[1] + 1))
            read = rand_seq(rng, L)
            if with_n and rng.random() < 0.1:
                p = int(rng.integers(0, L))
                read = read[:p] + "N" + read[p + 1:]
            start = int(rng.integers(0, max(1, len(tmpl[names[entry]]) - L + 4)))
            counts = (rng.integers(0, 4, S) * rng.integers(0, 30, S)).tolist()
            if exact_items:
                counts = [0] * S
                counts[int(rng.integers(0, S))] = int(rng.integers(1, 40))
        if read in seen or not 1 <= len(read) <= 255:
            prev = None                                                  # (a variant that exists already: draw afresh)
            continue
        seen.add(read)
        kind = trf.KIND_NONE if len(reads) % 11 == 5 else int(rng.integers(0, 3))
        reads.append(read)
        quant.append(counts)
        rows.append((len(reads) - 1, entry, start, int(rng.integers(0, 7)), kind))
        prev = (read, entry, start, counts) if kind != trf.KIND_NONE else None
    denom = [int(sum(q[s] for q in quant)) + 17 for s in range(S)]
    return arrays_of(names, ["A%d" % (i % 9) for i in range(len(names))], tables, pre, ["s%d.fastq" % s for s in range(S)], denom,
                     reads, quant, rows)


@pytest.mark.parametrize("world", WORLDS)
def test_golden_worlds(engine, golden, world, tmp_path):  # noqa: F811
    a = golden_arrays(golden, world, str(tmp_path / "libs"))
    timings = {}
    got, _ = assert_equal_to_model(engine, a, timings)
    assert got.G > 0 and {"groups_count_ms", "groups_fill_ms", "items_kernel_ms", "read_order_kernel_ms", "row_order_kernel_ms",
                          "pack_kernel_ms"} <= set(timings)


def test_hand_made_world(engine):
    got, _ = assert_equal_to_model(engine, hand_world())
    assert got.max_len == 255 and got.has_n
    got, _ = assert_equal_to_model(engine, hand_world(long_template=256))
    assert got.max_len == 256 and not got.filled
    got, want = assert_equal_to_model(engine, hand_world(missing=True))
    assert got.no_template_row is not None and not got.filled


def test_random_world_with_n(engine):
    got, _ = assert_equal_to_model(engine, random_world(1, 3000, 3, 40, (16, 45), (60, 110), True))
    assert got.has_n and got.G > 60 and got.n > 5000


@pytest.mark.parametrize("W,read_len,tmpl_len", [(1, (16, 31), (20, 32)), (2, (16, 63), (70, 96)), (4, (16, 127), (100, 160)),
                                                   (8, (16, 254), (200, 255))])
@pytest.mark.parametrize("with_n", (True, False))
def test_every_read_width(engine, W, read_len, tmpl_len, with_n):
    a = random_world(10 * W + with_n, 400, 2, 6, read_len, tmpl_len, with_n)
    assert a.words.shape[0] == W and (a.nmask is not None) == with_n
    got, _ = assert_equal_to_model(engine, a)
    assert got.has_n == with_n and got.n > 50


@pytest.mark.parametrize("n_items", (1, 63, 64, 65, 70001))
def test_item_counts_around_the_wave_and_beyond_one_tile(engine, n_items):
    a = random_world(n_items, n_items + n_items // 6 + 6, 2, 12, (16, 30), (60, 90), n_items < 100, exact_items=True)
    classified = int((a.rec[:, 7] <= trf.KIND_DELE).sum())
    keep = np.nonzero(a.rec[:, 7] <= trf.KIND_DELE)[0][n_items:]            # exactly n_items classified rows
    a.rec[keep, 7] = trf.KIND_NONE
    assert classified >= n_items and (a.rec[:, 7] == trf.KIND_NONE).any() and a.words.shape[1] > a.rec.shape[0]
    got, _ = assert_equal_to_model(engine, a)
    assert got.n_items == n_items


def test_counting_call_alone(engine):
    a = hand_world()
    want = model_groups(a.st, a.rec, a.words, a.lens, a.nmask, a.quant, a.denom)
    import torch
    dev = lambda x, v: torch.from_numpy(np.ascontiguousarray(x).view(v)).to(engine.device)
    words, lens, nmask = dev(a.words, np.int64), dev(a.lens, np.uint8), dev(a.nmask, np.int64)
    quant, rec = dev(a.quant, np.int32), dev(a.rec, np.int32)
    entries = np.ascontiguousarray(a.st.entries, dtype=np.int32)
    counts = (C.c_uint64 * 8)()
    W, n = a.words.shape
    rc = engine._lib.mrg_trf_sample_groups(
        engine._h, words.data_ptr(), W, n, lens.data_ptr(), nmask.data_ptr(), n, quant.data_ptr(), 3, rec.data_ptr(),
        a.rec.shape[0], a.denom.ctypes.data, entries.ctypes.data, entries.shape[0], a.st.n_names, 0, 0, None, None, None, None,
        None, None, None, None, None, counts, None, engine._stream_ptr())
    assert rc == 0
    assert list(counts)[:7] == [want.n_items, len(want.blocks), want.G, want.n, 255, 1, 0xFFFFFFFF]
    assert counts[7] == max(len(a.reads[r[0]]) for r in a.rec.tolist() if r[7] <= trf.KIND_DELE)
    # a filling call whose buffers are too small is refused, nothing is written
    blocks = np.zeros((2, 6), dtype=np.int32)
    x = words.data_ptr()
    rc = engine._lib.mrg_trf_sample_groups(
        engine._h, words.data_ptr(), W, n, lens.data_ptr(), nmask.data_ptr(), n, quant.data_ptr(), 3, rec.data_ptr(),
        a.rec.shape[0], a.denom.ctypes.data, entries.ctypes.data, entries.shape[0], a.st.n_names, 2, 2, blocks.ctypes.data,
        blocks.ctypes.data, blocks.ctypes.data, blocks.ctypes.data, x, x, x, x, x, counts, None, engine._stream_ptr())
    assert rc < 0 and b"count first" in engine._lib.mrg_last_error() and not blocks.any()


def stable_rank(off, rho):
    rank = np.zeros(len(rho), dtype=np.uint32)
    for a, b in zip(off[:-1].astype(int), off[1:].astype(int)):
        rank[a:b] = np.argsort(-rho[a:b], kind="stable")
    return rank


def test_rank_equals_the_stable_argsort(engine):
    rng = np.random.default_rng(2024)
    lens = (72, 255, 40, 76, 255, 90, 255, 76, 200, 255)
    specs = [(n, lens[k], k in (4, 7)) for k, n in enumerate((1, 2, 3, 63, 64, 65, 255, 256, 257, 4096))]
    specs.append((300, 120, True))                                   # all RPM equal: rank ties everywhere
    args = trf_samples.layout([trf_samples.Group(random_rows(rng, n, L, eq)) for n, L, eq in specs])
    got = engine.trf_peaks(*args, trf_samples.gaussian_table())
    rank = got.rank()
    want = stable_rank(args[0], got.rho)
    assert np.array_equal(rank, want)
    assert all(np.array_equal(x, y) for x, y in zip(got.min_distance(None), got.min_distance(want)))


def test_peaks_on_the_device_layout(engine, golden, tmp_path):  # noqa: F811
    a = golden_arrays(golden, "large", str(tmp_path / "libs"))
    g = engine.trf_sample_groups(a.st, a.rec, a.words, a.lens, a.nmask, a.quant, a.denom)
    kt = trf_samples.gaussian_table()
    p1 = engine.trf_peaks_groups(g, kt)
    p2 = engine.trf_peaks(g.off, g.codes, g.nmask, g.span, g.rpm, g.max_len, kt)
    assert np.array_equal(p1.rho.view(np.uint32), p2.rho.view(np.uint32)) and np.array_equal(p1.max_dis, p2.max_dis)
    rank = p1.rank()
    assert np.array_equal(rank, stable_rank(g.off, p2.rho))
    assert all(np.array_equal(x, y) for x, y in zip(p1.min_distance(None), p2.min_distance(rank)))


@pytest.mark.parametrize("world", WORLDS)
def test_cli_trf_without_a_python_object_per_read(golden, world, tmp_path, monkeypatch):  # noqa: F811
    from mirge_amd import cli, synth
    t, w = golden["trf"], golden["worlds"][world]
    root = str(tmp_path / "libs")
    ns = types.SimpleNamespace(libs={k: tuple(v) for k, v in t["libraries"].items()}, merges=t["merges"])
    synth.SynthLibraries.write_layout(ns, root, species="human", db="miRBase")
    for suffix, text in t["tables"].items():
        with open(os.path.join(root, "human", "annotation.Libs", "human" + suffix), "w") as fh:
            fh.write(text)
    samples = t["samples"] if world == "small" else [[r[0] for r in w["reads"] for _ in range(r[1 + i])] for i in range(2)]
    fastqs = []
    for name, reads in zip(w["sample_list"], samples):
        fastqs.append(str(tmp_path / name))
        with open(fastqs[-1], "w") as fh:
            fh.write("".join("@r%d\n%s\n+\n%s\n" % (k, r, "I" * len(r)) for k, r in enumerate(reads)))

    def run(out, *extra):
        res = cli.annotate_main(cli.build_parser().parse_args(
            ["annotate", "-s"] + fastqs + ["-lib", root, "-sp", "human", "-o", str(tmp_path / out), "-trf"] + list(extra)))
        return os.path.join(res["outdir"], "tRFs.samples.tmp")
    host = run("host", "--trf-host")

    def refuse(*a, **k):
        raise AssertionError("the array route built a Python object per read")
    monkeypatch.setattr(trf, "content_from_rows", refuse)
    monkeypatch.setattr(trf_samples, "sample_trf_dic", refuse)
    tdir = run("arrays")
    check_dir(w, tdir)
    for fn in os.listdir(host):
        with open(os.path.join(host, fn), "rb") as f1, open(os.path.join(tdir, fn), "rb") as f2:
            assert f1.read() == f2.read(), fn
