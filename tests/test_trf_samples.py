"""mirge_amd.trf_samples (the per-sample tRF reports and density-peak clusters of `-trf`, W2C:802-1088) against
the reference's own files (tests/golden/trf_samples.json) with the CPU model of the device arrays
(tests/trf_peaks_model.py) as the backend; the model against a transcription of the reference's getDistance /
local_density / min_distance; argument checks of the C-ABI."""
import base64
import ctypes as C
import json
import math
import os
import zlib

import numpy as np
import pytest

from mirge_amd import trf, trf_samples
from tests.conftest import ROOT
from tests.trf_peaks_model import model_peaks, random_rows

WORLDS = ("small", "large")


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "trf_samples.json")) as fh:
        g = json.load(fh)
    with open(os.path.join(ROOT, "tests", "golden", "trf.json")) as fh:
        g["trf"] = json.load(fh)
    s = g["trf"]["samples"]            # the small world's reads are trf.json's
    g["worlds"]["small"]["reads"] = [[r, s[0].count(r), s[1].count(r)] for r in sorted(set(s[0] + s[1]))]
    return g


def tables_of(golden, root):
    t = golden["trf"]
    ann = os.path.join(root, "human", "annotation.Libs")
    os.makedirs(ann, exist_ok=True)
    for suffix, text in t["tables"].items():
        with open(os.path.join(ann, "human" + suffix), "w") as fh:
            fh.write(text)
    return trf.load_trf_tables(root, "human"), dict(zip(*t["libraries"]["pre_trna"]))


def content_of(w):
    """trfContentDic as writeDataToCSV leaves it at W2C:802: the reads' counts, RPM as write_trf_tables makes it."""
    denom = [q["maturetrnaReads"] + q["pretrnaReads"] for q in w["quantStats"]]
    out = {}
    for ri, ni, start, ti in w["trfContentDic"]:
        read, counts = w["reads"][ri][0], w["reads"][ri][1:]
        out[read] = {"uid": "", "count": counts, "RPM": [100000.0 * c / d if d else 0.0 for c, d in zip(counts, denom)],
                     w["trf_names"][ni]: {"tRFType": w["trf_types"][ti], "start": start, "cigar": "undifined"}}
    return out


def expected_files(w):
    return {k: zlib.decompress(base64.b64decode(v)).decode() for k, v in w["files_z"].items()}


def check_dir(w, tdir):
    want = expected_files(w)
    assert sorted(os.listdir(tdir)) == sorted(want)
    for fn, text in want.items():
        with open(os.path.join(tdir, fn)) as fh:
            assert fh.read() == text, fn


@pytest.mark.parametrize("world", WORLDS)
def test_files_equal_the_reference(golden, world, tmp_path):
    w = golden["worlds"][world]
    tables, pre = tables_of(golden, str(tmp_path / "libs"))
    borders = []

    def peaks(*a):
        m = model_peaks(*a)
        border = m.border
        m.border = lambda *b: borders.append(border(*b)) or borders[-1]
        return m
    tdir = trf_samples.write_trf_samples(str(tmp_path), w["sample_list"], content_of(w), tables, pre, peaks)
    check_dir(w, tdir)
    assert world == "small" or any((b > 0).any() for b in borders)   # NCLUST > 1, non-zero border densities


def test_large_world_covers_the_quirks(golden):
    """Several clusters with halos, a group without center (label -1), rows with N, one- and two-row blocks,
    blocks of 200+ rows, an empty block (its rows all overhang the template)."""
    files = expected_files(golden["worlds"]["large"])
    det = files["t0.fastq.potential_tRFs.clusters.detail"].split("\n")
    n_clusters = [int(x.split(": ")[1]) for x in det if x.startswith("Number of Clusters")]
    assert max(n_clusters) >= 3 and 0 in n_clusters
    assert max(int(x.split("Halo: ")[-1]) for x in det if x.startswith("Cluster:")) > 0
    sizes, cur, has_n = [], 0, False
    for line in files["t0.fastq.potential_tRFs.report"].split("\n"):
        if "RP100K sum:" in line:
            cur = 0
        elif "mature tRNA" in line or "primary tRNA trailer" in line:
            sizes.append(cur)
        elif line:
            cur += 1
            has_n |= "N" in line.split("\t")[0]
    assert has_n and {0, 1, 2} <= set(sizes) and max(sizes) >= 200


# ---------------------------------------------------------------- the model against the reference's loops
def ref_get_distance(info):
    """getDistance (W2C:417-449), transcribed."""
    dist, max_dis = {}, 0.0
    ids = list(info.keys())
    for i in range(len(ids)):
        for j in range(i + 1, len(ids)):
            s1, s2 = info[ids[i]]["allignedSeq"], info[ids[j]]["allignedSeq"]
            c1, c2 = trf.coordinate(s1), trf.coordinate(s2)
            sub = sum(1 for k in range(len(s1)) if s1[k] != "-" and s2[k] != "-" and s1[k] != s2[k])
            d = 1.0 * abs(c1[0] - c2[0]) + 1.0 * abs(c1[1] - c2[1]) + 1.0 * sub
            max_dis = max(max_dis, d)
            dist[(ids[i], ids[j])] = dist[(ids[j], ids[i])] = d
    for i in ids:
        dist[(i, i)] = 0.0
    return dist, max_dis, max(ids)


def ref_local_density(dist, info, max_id, dc):
    """local_density (W2C:470-499, gaussian), transcribed."""
    rho = [-1] + [0] * max_id
    for i in range(1, max_id):
        for j in range(i + 1, max_id + 1):
            rho[i] += math.exp(-(dist[(i, j)] / dc) ** 2) * info[j]["RPM"]
            rho[j] += math.exp(-(dist[(i, j)] / dc) ** 2) * info[i]["RPM"]
    for i in range(1, max_id + 1):
        rho[i] = rho[i] + info[i]["RPM"]
    return np.array(rho, np.float32)


def ref_min_distance(dist, max_dis, max_id, rho):
    """min_distance (W2C:509-533), transcribed with the pinned (stable) rank order."""
    order = np.argsort(-rho, kind="stable")
    delta, nneigh = [0.0] + [float(max_dis)] * (len(rho) - 1), [0] * len(rho)
    delta[order[0]] = -1.0
    for i in range(1, max_id):
        for j in range(0, i):
            if dist[(order[i], order[j])] <= delta[order[i]]:
                delta[order[i]], nneigh[order[i]] = dist[(order[i], order[j])], order[j]
    delta[order[0]] = max(delta)
    return np.array(delta, np.float32), np.array(nneigh, np.int32), order


@pytest.mark.parametrize("n,L,equal", [(1, 40, False), (2, 40, True), (5, 30, False), (37, 76, False),
                                       (40, 200, True), (60, 255, False)])
def test_model_equals_reference_loops(n, L, equal):
    rows = random_rows(np.random.default_rng(n * 1000 + L), n, L, equal)
    info = {k + 1: {"allignedSeq": r[0], "RPM": r[3]} for k, r in enumerate(rows)}
    dist, max_dis, max_id = ref_get_distance(info)
    rho_ref = ref_local_density(dist, info, max_id, 3.0)
    delta_ref, nn_ref, order = ref_min_distance(dist, max_dis, max_id, rho_ref)
    m = model_peaks(*trf_samples.layout([trf_samples.Group(rows)]), trf_samples.gaussian_table())
    assert np.array_equal(m.rho, rho_ref[1:]) and int(m.max_dis[0]) == max_dis
    assert all(m.D[0][i, j] == dist[(i + 1, j + 1)] for i in range(n) for j in range(n))
    assert order[-1] == 0
    delta, nneigh = m.min_distance(order[:-1] - 1)
    for k in range(n):
        if k == order[0] - 1:
            assert delta[k] == -1 and nneigh[k] == -1
        else:
            assert delta[k] == delta_ref[k + 1] and nneigh[k] + 1 == nn_ref[k + 1]


def test_gaussian_table_is_pythons():
    k = trf_samples.gaussian_table()
    assert len(k) == 82 and k[81] > 0.0 and math.exp(-(82 / 3.0) ** 2) == 0.0
    assert all(k[d] == math.exp(-(d / 3.0) ** 2) for d in range(82))


# ---------------------------------------------------------------- C-ABI argument checks (no GPU needed)
def test_trf_entry_points_refuse_bad_arguments(native_lib):
    L = native_lib
    off, bad_off = (C.c_uint32 * 3)(0, 2, 5), (C.c_uint32 * 3)(0, 4, 2)
    kt = (C.c_double * 4)(1.0, 0.5, 0.2, 0.1)
    bo, bad_bo = (C.c_uint32 * 3)(0, 0, 3), (C.c_uint32 * 3)(1, 0, 3)
    x = C.c_void_p(8)   # (a non-null pointer, never dereferenced: every call below fails its checks first)
    assert L.mrg_trf_rho(None, off, 2, 76, x, None, x, x, kt, 4, x, x, None) < 0
    assert b"null" in L.mrg_last_error()
    for args in ((x, None, 2, 76), (x, off, 2, 256), (x, off, 2, 0), (x, bad_off, 2, 76)):
        assert L.mrg_trf_rho(*args, x, None, x, x, kt, 4, x, x, None) < 0
    assert L.mrg_trf_rho(x, off, 2, 300, x, None, x, x, kt, 4, x, x, None) < 0 and b"255" in L.mrg_last_error()
    assert L.mrg_trf_rho(x, off, 2, 76, x, None, x, x, None, 4, x, x, None) < 0
    assert L.mrg_trf_rho(x, off, 2, 76, x, None, x, x, kt, 0, x, x, None) < 0
    assert L.mrg_trf_rho(x, off, 2, 76, x, None, x, x, kt, 4, None, x, None) < 0
    assert L.mrg_trf_delta(None, off, 2, 76, x, None, x, x, x, x, x, None) < 0
    assert L.mrg_trf_delta(x, off, 2, 76, x, None, x, None, x, x, x, None) < 0
    assert L.mrg_trf_delta(x, off, 0, 76, x, None, x, x, x, x, x, None) < 0
    assert L.mrg_trf_border(None, off, 2, 76, x, None, x, x, x, bo, x, None) < 0
    for b, rho, out in ((None, x, x), (bo, None, x), (bo, x, None), (bad_bo, x, x)):
        assert L.mrg_trf_border(x, off, 2, 76, x, None, x, rho, x, b, out, None) < 0


def test_host_refuses_long_templates():
    with pytest.raises(ValueError, match="255"):
        trf_samples.run_peaks([trf_samples.Group([("A" * 256, "x", 1, 1.0)])], model_peaks)
