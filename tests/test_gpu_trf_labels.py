"""Cluster centres, labels and halos of `-trf` on the GPU: TrfPeaks.assign() / .halo() (csrc/trf_labels.hip through
mrg_trf_assign / mrg_trf_halo) field by field against the model (tests/trf_labels_model.py) on the worlds of
tests/test_trf_labels.py; the entry points on hand-made forests (group sizes around the wave, a star, a path of 70 001 rows,
many small groups beside a large one, every row width); foreign arrays that name a row outside the group or run in a cycle;
border(None, ...) against border(labels, ...); `annotate -trf` end to end with the per-group Python made to raise."""
import os
import time
import types

import numpy as np
import pytest

from mirge_amd import trf, trf_samples
from tests.test_trf_labels import KTAB, World, golden_world, hand_world
from tests.test_trf_samples import WORLDS, check_dir, golden  # noqa: F401  (golden: the module fixture)
from tests.trf_peaks_model import random_rows

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine(native_lib):
    from mirge_amd.engine import Engine
    return Engine(0)


def upload(engine, a, dtype):
    import torch
    signed = {np.dtype(np.uint32): np.int32}
    a = np.ascontiguousarray(a if len(a) else np.zeros(1), dtype=dtype)
    return torch.from_numpy(a.view(signed.get(a.dtype, a.dtype))).to(engine.device)


class ForestState:
    """A TrfPeaks whose rho, rank, delta and nneigh are given by hand (World.forest), for World.arrays."""

    def __init__(self, engine, t, forest):
        self.t = t
        rho, rank, delta, nneigh = forest
        t.rho_d, t.rank_d = upload(engine, rho, np.float32), upload(engine, rank, np.uint32)
        t.delta_d, t.nneigh_d = upload(engine, delta, np.int32), upload(engine, nneigh, np.int32)
        self.rank = self.min_distance = lambda *a: None
        self.assign, self.border, self.halo, self.labels = t.assign, t.border, t.halo, t.labels


def engine_arrays(engine, w):
    t = engine.trf_peaks(w.off, w.codes, w.nmask, w.span, w.rpm, w.max_len, KTAB)
    return w.arrays(ForestState(engine, t, w.forest) if w.forest is not None else t)


def assert_same_arrays(got, want):
    for f in ("nclust", "cen_off", "centers", "labels", "core", "order", "tallies", "bord_off"):
        assert np.array_equal(np.asarray(getattr(got, f)), np.asarray(getattr(want, f))), f
    assert np.array_equal(np.asarray(got.bord).view(np.uint32), np.asarray(want.bord).view(np.uint32))


@pytest.mark.parametrize("name", WORLDS + ("hand",))
def test_assign_and_halo_equal_the_model(engine, golden, name, tmp_path):  # noqa: F811
    w = hand_world() if name == "hand" else golden_world(golden, name, str(tmp_path / "libs"))
    got, want = engine_arrays(engine, w), w.arrays()
    assert_same_arrays(got, want)
    assert got.labels.dtype == np.int32 and got.core.dtype == np.uint8 and got.tallies.shape == (len(want.centers), 4)
    if name == "hand":      # and the files from the device's arrays
        ref = w.reference()
        assert w.write(str(tmp_path / "new"), got) == w.reference_files(str(tmp_path / "ref"), ref)


@pytest.mark.parametrize("L", (30, 60, 120, 250))
def test_every_row_width(engine, L):
    rng = np.random.default_rng(L)
    fix = lambda rows: [(r[0], "i-tRF", int(rng.integers(1, 50)), r[3]) for r in rows]
    groups = [trf_samples.Group(fix(random_rows(rng, n, L))) for n in (40, 1, 130, 7)]
    w = World(["s"], [(0, "t%d" % k, g) for k, g in enumerate(groups)], {}, {})
    assert (w.max_len + 31) // 32 == {30: 1, 60: 2, 120: 4, 250: 8}[L] and w.nmask is not None
    got, want = engine_arrays(engine, w), w.arrays()
    assert_same_arrays(got, want)
    assert want.core.any() and not want.core.all() and (want.nclust > 1).any()


# ---------------------------------------------------------------- the entry point on forests given directly
def call_assign(engine, off, rho, rank, delta, nneigh):
    import torch
    off = np.ascontiguousarray(off, dtype=np.uint32)
    G, n = len(off) - 1, int(off[-1])
    dev = [upload(engine, a, dt) for a, dt in ((rho, np.float32), (rank, np.uint32), (delta, np.int32), (nneigh, np.int32))]
    label = torch.full((max(n, 1),), 77, dtype=torch.int32, device=engine.device)
    nclust, cen_off, centers = np.full(G, 99, np.uint32), np.full(G + 1, 99, np.uint32), np.full(max(n, 1), 99, np.uint32)
    import ctypes as C
    rc = engine._lib.mrg_trf_assign(engine._h, off.ctypes.data_as(C.POINTER(C.c_uint32)), G, *[d.data_ptr() for d in dev], label.data_ptr(),
                                    nclust.ctypes.data, n, cen_off.ctypes.data, centers.ctypes.data, engine._stream_ptr())
    return rc, label.cpu().numpy()[:n], nclust, cen_off, centers


def random_forest(rng, n, p_centre=0.1):
    """rank = a random order; every row but the top hangs on a row ranked above it; centres by rho / delta."""
    rank = rng.permutation(n).astype(np.uint32)
    nneigh, delta = np.full(n, -1, np.int32), np.full(n, -1, np.int32)
    for p in range(1, n):
        nneigh[rank[p]] = rank[int(rng.integers(0, p))]
        delta[rank[p]] = 20 if rng.random() < p_centre else int(rng.integers(0, 8))
    rho = np.where(rng.random(n) < 0.7, 9.0, 2.0).astype(np.float32)
    return rho, rank, delta, nneigh


def expected(off, rho, rank, delta, nneigh):
    """The definition, in rank order (W2C:883-912): (labels, nclust, centres)."""
    labels, nclust, centres = np.zeros(int(off[-1]), np.int32), [], []
    for a, b in zip(off[:-1].astype(int), off[1:].astype(int)):
        if a == b:
            nclust.append(0)
            continue
        d = delta[a:b].astype(np.int64)
        top = int(rank[a])
        d[top] = max(0, int(np.delete(d, top).max())) if b - a > 1 else 0
        cen = np.nonzero((rho[a:b] >= np.float32(5)) & (d >= 8))[0]
        if not len(cen) and d.max() <= 8 and rho[a:b].max() >= 5:
            cen = np.array([int(np.argmax(rho[a:b]))])
        lab = np.full(b - a, -1, np.int64)
        lab[cen] = np.arange(1, len(cen) + 1)
        nn = nneigh[a:b].tolist()
        lab_l, is_c = lab.tolist(), set(cen.tolist())
        for p, s in enumerate(rank[a:b].tolist()):
            if s not in is_c and p:
                lab_l[s] = lab_l[nn[s]]
        labels[a:b] = lab_l
        nclust.append(len(cen))
        centres += cen.tolist()
    return labels, np.array(nclust, np.uint32), np.array(centres, np.uint32)


def check_forests(engine, forests):
    off = np.zeros(len(forests) + 1, dtype=np.uint32)
    off[1:] = np.cumsum([len(f[0]) for f in forests])
    flat = [np.concatenate([f[k] for f in forests]) for k in range(4)]
    rc, label, nclust, cen_off, centers = call_assign(engine, off, *flat)
    assert rc == 0, engine._lib.mrg_last_error()
    want_l, want_n, want_c = expected(off, *flat)
    assert np.array_equal(nclust, want_n) and np.array_equal(np.diff(cen_off.astype(np.int64)), want_n) and cen_off[0] == 0
    assert np.array_equal(centers[:len(want_c)], want_c) and np.array_equal(label, want_l)
    return label, nclust


def test_group_sizes_around_the_wave(engine):
    rng = np.random.default_rng(7)
    label, nclust = check_forests(engine, [random_forest(rng, n) for n in (1, 2, 63, 64, 65, 257)])
    assert (label == -1).any() and nclust.max() >= 3


def test_star_and_path(engine):
    n = 300
    star = (np.full(n, 2.0, np.float32), np.arange(n, dtype=np.uint32), np.full(n, 3, np.int32), np.zeros(n, np.int32))
    star[0][0], star[3][0] = 9.0, -1                                  # the top alone is dense: the fallback centre
    m = 70_001                                                        # 17 doublings; labels travel from several centres
    rho = np.full(m, 2.0, np.float32)
    delta = np.full(m, 1, np.int32)
    cen = np.array([5, 6, 4000, 20_000, 20_001, 65_536, 70_000])      # (the top, row 0, is none: rows 0..4 get -1)
    rho[cen], delta[cen] = 7.5, 8
    path = (rho, np.arange(m, dtype=np.uint32), delta, np.arange(-1, m - 1, dtype=np.int32))
    label, nclust = check_forests(engine, [star, path])
    assert nclust.tolist() == [1, 7] and (label[:n] == 1).all()
    p = label[n:]
    assert (p[:5] == -1).all() and p[5] == 1 and (p[6:4000] == 2).all() and (p[20_001:65_536] == 5).all() and p[-1] == 7 and p[-2] == 6


def test_many_small_groups_beside_a_large_one(engine):
    rng = np.random.default_rng(11)
    forests = [random_forest(rng, int(n)) for n in rng.integers(1, 6, 400)]
    forests.insert(200, random_forest(rng, 5000, 0.01))
    label, nclust = check_forests(engine, forests)
    assert (nclust == 0).any() and nclust.max() >= 10


def test_foreign_arrays_are_refused(engine):
    """Input validation of a C-ABI call that takes foreign arrays: an index outside the group is never followed, and rows that
    reach no root in the fixed number of rounds (a cycle) end the call with an error, without output."""
    rng = np.random.default_rng(13)
    forests = [random_forest(rng, n) for n in (40, 300, 9)]
    off = np.array([0, 40, 340, 349], dtype=np.uint32)

    def broken(change):
        flat = [np.concatenate([f[k] for f in forests]) for k in range(4)]
        change(*flat)
        t0 = time.perf_counter()
        rc, label, nclust, cen_off, centers = call_assign(engine, off, *flat)
        assert time.perf_counter() - t0 < 5.0
        assert rc < 0 and not label.any()                                              # (0 is no label)
        assert (nclust == 99).all() and (cen_off == 99).all() and (centers == 99).all()   # nothing reported
        return engine._lib.mrg_last_error()

    def outside(rho, rank, delta, nneigh):
        rho[40 + int(forests[1][1][17])] = 1.0                                          # (no centre: its nneigh counts)
        nneigh[40 + int(forests[1][1][17])] = 300                                       # a row of the next group
    assert b"outside its group" in broken(outside)

    def negative(rho, rank, delta, nneigh):
        rho[40 + int(forests[1][1][17])] = 1.0
        nneigh[40 + int(forests[1][1][17])] = -5
    assert b"outside its group" in broken(negative)

    def cycle(rho, rank, delta, nneigh):
        i, j = (40 + int(forests[1][1][p]) for p in (100, 200))                         # neither is the top
        rho[[i, j]] = 1.0                                                               # ... nor a centre
        nneigh[i], nneigh[j] = j - 40, i - 40
    assert b"cycle" in broken(cycle)

    def top(rho, rank, delta, nneigh):
        rank[40] = 300
    assert b"rank" in broken(top)
    # the same arrays, unbroken, pass
    check_forests(engine, forests)


def test_halo_refuses_labels_that_name_no_cluster(engine):
    w = hand_world()
    t = engine.trf_peaks(w.off, w.codes, w.nmask, w.span, w.rpm, w.max_len, KTAB)
    w.arrays(ForestState(engine, t, w.forest))
    import torch
    from mirge_amd._native import MirgeAmdError
    lab = t.labels().copy()
    lab[int(w.off[3]) + 2] = 4                                                          # NCLUST is 3
    t.label_d = torch.from_numpy(lab).to(engine.device)
    with pytest.raises(MirgeAmdError, match="no cluster"):
        t.halo(w.rows[:, 1])


def test_border_from_the_device_labels(engine, golden, tmp_path):  # noqa: F811
    w = golden_world(golden, "large", str(tmp_path / "libs"))
    t = engine.trf_peaks(w.off, w.codes, w.nmask, w.span, w.rpm, w.max_len, KTAB)
    x = w.arrays(t)
    again = t.border(x.labels, x.bord_off)
    assert x.bord_off[-1] > 0 and (x.bord > 0).any() and np.array_equal(again.view(np.uint32), np.asarray(x.bord).view(np.uint32))


# ---------------------------------------------------------------- annotate -trf
@pytest.mark.parametrize("world", WORLDS)
def test_cli_trf_without_python_per_group(golden, world, tmp_path, monkeypatch):  # noqa: F811
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
        raise AssertionError("the array route walked the groups in Python")
    monkeypatch.setattr(trf_samples, "cluster_text", refuse)
    monkeypatch.setattr(trf_samples, "peaks_results", refuse)
    monkeypatch.setattr(trf, "content_from_rows", refuse)
    tdir = run("arrays")
    check_dir(w, tdir)
    for fn in os.listdir(host):
        with open(os.path.join(host, fn), "rb") as f1, open(os.path.join(tdir, fn), "rb") as f2:
            assert f1.read() == f2.read(), fn
