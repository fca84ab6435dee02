"""The density-peak passes of `-trf` on the GPU (csrc/trf_peaks.hip through Engine.trf_peaks) bit-equal to the
CPU model (tests/trf_peaks_model.py), and `annotate -trf` end to end writing the reference's
tRFs.samples.tmp/ files (tests/golden/trf_samples.json)."""
import os
import types

import numpy as np
import pytest

from mirge_amd import trf_samples
from tests.test_trf_samples import WORLDS, check_dir, golden  # noqa: F401  (golden: the module fixture)
from tests.trf_peaks_model import ModelPeaks, decode, distances, random_rows, rho_of

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine(native_lib):
    from mirge_amd.engine import Engine
    return Engine(0)


def layout(rng, specs):
    return trf_samples.layout([trf_samples.Group(random_rows(rng, n, L, eq)) for n, L, eq in specs])


def stable_rank(off, rho):
    rank = np.zeros(len(rho), dtype=np.uint32)
    for a, b in zip(off[:-1].astype(int), off[1:].astype(int)):
        rank[a:b] = np.argsort(-rho[a:b], kind="stable")
    return rank


def test_peaks_bit_equal_to_the_model(engine):
    rng = np.random.default_rng(2024)
    lens = (72, 255, 40, 76, 255, 90, 255, 76, 200, 255)
    specs = [(n, lens[k], k in (4, 7)) for k, n in enumerate((1, 2, 3, 63, 64, 65, 255, 256, 257, 4096))]
    specs.append((300, 120, True))                                   # all RPM equal: rank ties everywhere
    off, codes, nmask, span, rpm, max_len = layout(rng, specs)
    kt = trf_samples.gaussian_table()
    assert nmask is not None
    for nm in (nmask, None):                                         # both kernel instantiations
        got = engine.trf_peaks(off, codes, nm, span, rpm, max_len, kt)
        want = ModelPeaks(off, codes, nm, span, rpm, max_len, kt)
        assert np.array_equal(got.rho.view(np.uint32), want.rho.view(np.uint32))
        assert np.array_equal(got.max_dis, want.max_dis)
        rank = stable_rank(off, want.rho)
        assert all(np.array_equal(a, b) for a, b in zip(got.min_distance(rank), want.min_distance(rank)))
    labels = rng.integers(-1, 4, int(off[-1])).astype(np.int32)
    labels[labels == 0] = 1
    slots = [4 if g % 3 else 0 for g in range(len(off) - 1)]
    slots[1] = 2                                                     # NCLUST = 1: skipped
    bord_off = np.concatenate([[0], np.cumsum(slots)]).astype(np.uint32)
    b1, b2 = got.border(labels, bord_off), want.border(labels, bord_off)
    assert (b2 > 0).any() and np.array_equal(b1.view(np.uint32), b2.view(np.uint32))


def test_refuses_templates_longer_than_255(engine):
    from mirge_amd._native import MirgeAmdError
    with pytest.raises(MirgeAmdError, match="255"):
        engine.trf_peaks(np.array([0, 1], np.uint32), np.zeros((9, 1), np.uint64), None,
                         np.array([1 | (1 << 8)], np.uint16), np.ones(1), 256, trf_samples.gaussian_table())


def test_group_of_20000_rows_on_sampled_rows(engine):
    rng = np.random.default_rng(77)
    off, codes, nmask, span, rpm, max_len = layout(rng, [(20000, 76, False)])
    kt = trf_samples.gaussian_table()
    got = engine.trf_peaks(off, codes, nmask, span, rpm, max_len, kt)
    rank = stable_rank(off, got.rho)
    delta, nneigh = got.min_distance(rank)
    ch, f, l = decode(codes, nmask, span, np.arange(20000), (max_len + 31) // 32)
    pos = np.empty(20000, dtype=np.int64)
    pos[rank] = np.arange(20000)
    for i in rng.choice(20000, 256, replace=False):
        d = distances(ch[i:i + 1], f[i:i + 1], l[i:i + 1], ch, f, l)[0]
        assert rho_of(d, i, rpm, kt).view(np.uint32) == got.rho[i].view(np.uint32)
        assert int(np.delete(d, i).max()) <= int(got.max_dis[0])
        p = pos[i]
        if p == 0:
            assert delta[i] == -1 and nneigh[i] == -1
            continue
        cand = d[rank[:p]]
        m = min(int(cand.min()), int(got.max_dis[0]))
        assert (delta[i], nneigh[i]) == (m, rank[p - 1 - int(np.argmax(cand[::-1] == m))])


@pytest.mark.parametrize("world", WORLDS)
def test_cli_trf_writes_the_reference_sample_files(golden, world, tmp_path):  # noqa: F811
    from mirge_amd import cli, synth
    t, w = golden["trf"], golden["worlds"][world]
    root = str(tmp_path / "libs")
    ns = types.SimpleNamespace(libs={k: tuple(v) for k, v in t["libraries"].items()}, merges=t["merges"])
    synth.SynthLibraries.write_layout(ns, root, species="human", db="miRBase")
    for suffix, text in t["tables"].items():
        with open(os.path.join(root, "human", "annotation.Libs", "human" + suffix), "w") as fh:
            fh.write(text)
    samples = t["samples"] if world == "small" else [[r[0] for r in w["reads"] for _ in range(r[1 + i])]
                                                     for i in range(2)]
    fastqs = []
    for name, reads in zip(w["sample_list"], samples):
        fastqs.append(str(tmp_path / name))
        with open(fastqs[-1], "w") as fh:
            fh.write("".join("@r%d\n%s\n+\n%s\n" % (k, r, "I" * len(r)) for k, r in enumerate(reads)))
    out = cli.annotate_main(cli.build_parser().parse_args(
        ["annotate", "-s"] + fastqs + ["-lib", root, "-sp", "human", "-o", str(tmp_path / "out"), "-trf"]))
    check_dir(w, os.path.join(out["outdir"], "tRFs.samples.tmp"))
