"""Cluster centres, labels and halos of `-trf` from the arrays, without a GPU: the model of mrg_trf_assign / mrg_trf_halo
(tests/trf_labels_model.py) against peaks_results + cluster_text of mirge_amd/trf_samples.py on the golden worlds and on a
hand-made world whose forest is given directly, so that every branch occurs (asserted); the native writer
(mrg_write_trf_cluster_reports) against _write_clusters; write_trf_samples_arrays(device_labels=True) against the
reference's files; mrg_py3_float_repr against repr; argument checks of the C-ABI."""
import ctypes as C
import os
import types

import numpy as np
import pytest

from mirge_amd import trf, trf_samples
from tests.test_trf_groups import content_from, golden_arrays, hand_world as groups_hand_world
from tests.test_trf_samples import WORLDS, check_dir, content_of, expected_files, golden  # noqa: F401
from tests.trf_groups_model import model_groups
from tests.trf_labels_model import LabelsModel, model_label_peaks
from tests.trf_peaks_model import ModelPeaks

KTAB = trf_samples.gaussian_table()
TAGS = {"nclust0", "fallback", "nclust1", "nclust3", "minus_beside", "halo_border", "halo_far", "centre_not_top", "skipped",
        "one_row", "n_printed"}


# ---------------------------------------------------------------- worlds
class World:
    """Groups of the record route (trf_samples.Group) with the name and sample of each, as the arrays the device sees."""

    def __init__(self, sample_list, triples, stru, pre, forest=None):
        self.sample_list, self.stru, self.pre = list(sample_list), stru, pre
        self.sample = np.array([t[0] for t in triples], dtype=np.int32)
        self.names = [t[1] for t in triples]
        self.groups = [t[2] for t in triples]
        self.off, self.codes, self.nmask, self.span, self.rpm, self.max_len = trf_samples.layout(self.groups)
        self.n = int(self.off[-1])
        self.rows = np.zeros((self.n, 3), dtype=np.uint32)
        self.rows[:, 1] = [c for g in self.groups for c in g.counts]
        self.rows[:, 2] = [trf.TRF_TYPES.index(t) for g in self.groups for t in g.types]
        self.group_len = np.array([g.L for g in self.groups], dtype=np.int32)
        self.forest = forest(self) if forest else None

    def peaks(self):
        return LabelsModel(ModelPeaks(self.off, self.codes, self.nmask, self.span, self.rpm, self.max_len, KTAB), self.forest)

    def reference(self):
        """peaks_results and cluster_text of the record route: one (result, text, content, sum) per group."""
        res = trf_samples.peaks_results(self.off, self.peaks(), device_rank=True)
        return [(r,) + trf_samples.cluster_text(name, g, r) for name, g, r in zip(self.names, self.groups, res)]

    def arrays(self, state=None):
        """The arrays of the device_labels route from a backend (the model here, the engine in the GPU tests)."""
        state = state or self.peaks()
        state.rank()
        state.min_distance(None)
        nclust, cen_off, centers = state.assign()
        bord_off = np.zeros(len(self.groups) + 1, dtype=np.uint32)
        bord_off[1:] = np.cumsum(np.where(nclust > 1, nclust + 1, 0))
        bord = state.border(None, bord_off)
        core, order, tallies = state.halo(self.rows[:, 1])
        return types.SimpleNamespace(nclust=nclust, cen_off=cen_off, centers=centers, labels=state.labels(), core=core, order=order,
                                     tallies=tallies, bord=bord, bord_off=bord_off)

    def write(self, tdir, x):
        os.makedirs(tdir, exist_ok=True)
        trf_samples.write_trf_cluster_reports(tdir, self.sample_list, self, self.names, self.group_len, self.sample, self.stru,
                                              self.pre, x.labels, x.core, x.order, x.nclust, x.cen_off, x.centers, x.tallies)
        return read_files(tdir, self.sample_list)

    def reference_files(self, tdir, ref):
        os.makedirs(tdir, exist_ok=True)
        for si, s in enumerate(self.sample_list):
            trf_samples._write_clusters(tdir, s, [(self.names[k], self.groups[k], ref[k][0]) for k in np.nonzero(self.sample == si)[0]],
                                        self.stru, self.pre)
        return read_files(tdir, self.sample_list)


def read_files(tdir, sample_list):
    out = {}
    for s in sample_list:
        for suffix in (".potential_tRFs.clusters.detail", ".tRFs.report.tsv"):
            with open(os.path.join(tdir, s + suffix)) as fh:
                out[s + suffix] = fh.read()
    return out


def golden_world(golden, world, root):  # noqa: F811
    a = golden_arrays(golden, world, root)
    stru, aa = a.tables["trnaStruDic"], a.tables["trnaAAanticodonDic"]
    sdic = trf_samples.sample_trf_dic(content_of(golden["worlds"][world]), a.sample_list, stru, a.pre)
    triples = []
    for si, s in enumerate(a.sample_list):
        lines, _ = trf_samples.sample_reports(sdic[s], stru, aa, a.pre)
        names = [line.split("\t")[0] for line in lines if "RP100K sum:" in line]
        triples += [(si, names[k], trf_samples.Group(rows)) for k, rows in enumerate(trf_samples.load_data_new(lines))]
    return World(a.sample_list, triples, stru, a.pre)


def hand_world():
    """Two samples with groups (a third without): natural one-row groups, a stack with a far straggler, a trailer, and one
    group whose forest is written by hand (see `forest`)."""
    rng = np.random.default_rng(17)
    seq = lambda n: "".join("ACGT"[c] for c in rng.integers(0, 4, n))
    tmpl = {k: seq(76) for k in ("tA", "tB", "tC", "tD", "tE")}
    tmpl["tShort"] = seq(40)
    pre = {"pre_tA_trailer": seq(50), "pre_tF_trailer": seq(45)}

    def row(name, a, b, count, rpm, kind="i-tRF", subs=()):
        t = pre[name] if name in pre else tmpl[name]
        r = list(t[a:b])
        for p, ch in subs:
            r[p - a] = ch if ch != "x" else "ACGT"[("ACGT".index(t[p]) + 1) % 4]
        return ("-" * a + "".join(r) + "-" * (len(t) - b), kind, count, rpm)
    by_hand = [row("tC", 0, 30, 2, 1.25), row("tC", 0, 31, 40, 22.5, "5'-tRF"), row("tC", 0, 31, 9, 5.125, "5'-tRF", [(12, "x")]),
               row("tC", 1, 31, 4, 2.0), row("tC", 40, 70, 30, 17.001), row("tC", 40, 60, 6, 3.3),
               row("tC", 41, 70, 7, 4.0, "i-tRF", [(50, "N")]), row("tC", 0, 29, 1, 0.5)]
    stack = [row("tD", 0, 30, 50, 50.0, "5'-tRF"), row("tD", 0, 29, 5, 5.0, "5'-tRF"), row("tD", 1, 30, 4, 4.001, "5'-tRF", [(9, "x")]),
             row("tD", 42, 72, 1, 1.0)]
    trailer = [row("pre_tA_trailer", 20, 50, 12, 9.0, "tRF-1"), row("pre_tA_trailer", 21, 50, 3, 2.5, "tRF-1", [(30, "x")]),
               row("pre_tA_trailer", 22, 50, 2, 1.0, "tRF-1")]
    triples = [(0, "tA", trf_samples.Group([row("tA", 5, 35, 20, 20.0, "5'-tRF", [(7, "x")])])),
               (0, "tB", trf_samples.Group([row("tB", 5, 35, 1, 1.5)])),
               (0, "pre_tA_trailer", trf_samples.Group(trailer)),
               (0, "tC", trf_samples.Group(by_hand)),
               (0, "tD", trf_samples.Group(stack)),
               # (the pairing quirk: rows of a 40-nt template under the name of a 76-nt one)
               (1, "tE", trf_samples.Group([("-" * 4 + tmpl["tShort"][4:30] + "-" * 10, "i-tRF", 30, 30.0)])),
               (1, "pre_tF_trailer", trf_samples.Group([row("pre_tF_trailer", 25, 45, 11, 12.0, "tRF-1")])),
               (1, "tC", trf_samples.Group(by_hand[:3]))]

    def forest(w):
        """The passes' own arrays, and over the rows of the hand-made group: top = row 0 (rho 3: no centre, label -1, and row 7
        hangs on it); centres 1 = row 1, 2 = row 3 (one step from row 1 and far sparser: below its border density, so cluster
        2 has no core and is skipped), 3 = row 4; row 2 is dimmer than cluster 1's border, row 5 lies 10 from its centre, row 6
        holds an N.  Row 5's delta is 7 by hand: it must not become a centre."""
        m = LabelsModel(ModelPeaks(w.off, w.codes, w.nmask, w.span, w.rpm, w.max_len, KTAB))
        rho, rank = m.rho.copy(), m.rank().copy()
        delta, nneigh = (x.copy() for x in m.min_distance(None))
        a = int(w.off[3])
        rho[a:a + 8] = [3, 40, 20, 6, 30, 8, 25, 1]
        rank[a:a + 8] = [0, 1, 4, 2, 5, 3, 6, 7]
        delta[a:a + 8] = [-1, 9, 1, 8, 40, 7, 2, 1]
        nneigh[a:a + 8] = [-1, 0, 1, 1, 1, 4, 4, 0]
        return rho, rank, delta, nneigh
    stru = {k: {"seq": v} for k, v in tmpl.items()}
    return World(["s0.fastq", "s1.fastq", "s2.fastq"], triples, stru, pre, forest)


def tags_of(w, ref):
    """Which branches the record route takes on world w."""
    tags = set()
    for g, (r, text, _, _) in zip(w.groups, ref):
        nclust, cl, rho, delta = r["NCLUST"], r["cl"][1:], r["rho"][1:], r["delta"][1:]
        flagged = bool(((rho >= 5.0) & (delta >= 8.0)).any())
        tags |= {"one_row"} if g.n == 1 else set()
        tags |= {"nclust0"} if nclust == 0 else {"nclust1" if flagged else "fallback"} if nclust == 1 else set()
        tags |= {"nclust3"} if nclust >= 3 else set()
        tags |= {"minus_beside"} if nclust >= 1 and (cl == -1).any() else set()
        tags |= {"centre_not_top"} if any(c != int(r["sort_rho_idx"][0]) for c in r["ccenter"].values()) else set()
        tags |= {"skipped"} if int(text.split("Number of Clusters: ")[1].split("\n")[0]) < nclust else set()
        for c, idx in r["ccenter"].items():
            sel = np.nonzero(cl == c)[0]
            if (g.distance_to(idx - 1, sel) > 8).any():
                tags.add("halo_far")
            if nclust > 1 and (rho[sel] < r["bord_rho"][c]).any():
                tags.add("halo_border")
        body = [line.split("\t")[0] for line in text.split("\n") if line.count("\t") == 3]
        tags |= {"n_printed"} if any("N" in s for s in body) else set()
    return tags


@pytest.fixture(scope="module")
def worlds(golden, tmp_path_factory):  # noqa: F811
    out = {name: golden_world(golden, name, str(tmp_path_factory.mktemp("libs_" + name))) for name in WORLDS}
    out["hand"] = hand_world()
    return {k: (w, w.reference(), w.arrays()) for k, w in out.items()}


# ---------------------------------------------------------------- the model against the record route
def test_every_branch_occurs(worlds):
    seen = {k: tags_of(w, ref) for k, (w, ref, _) in worlds.items()}
    assert set().union(*seen.values()) == TAGS, seen
    assert seen["hand"] >= {"minus_beside", "skipped", "halo_border", "halo_far", "centre_not_top", "nclust3", "fallback",
                            "nclust1", "nclust0", "one_row", "n_printed"}


@pytest.mark.parametrize("name", WORLDS + ("hand",))
def test_model_equals_the_record_route(worlds, name):
    w, ref, x = worlds[name]
    assert x.labels.dtype == np.int32 and x.core.dtype == np.uint8 and len(x.order) == w.n
    for k, (g, (r, text, _, _)) in enumerate(zip(w.groups, ref)):
        a, b, c0 = int(w.off[k]), int(w.off[k + 1]), int(x.cen_off[k])
        assert int(x.nclust[k]) == r["NCLUST"] == int(x.cen_off[k + 1]) - c0, k
        assert np.array_equal(x.labels[a:b], r["cl"][1:]), k
        assert [int(c) + 1 for c in x.centers[c0:c0 + r["NCLUST"]]] == [r["ccenter"][c] for c in range(1, r["NCLUST"] + 1)], k
        # the text: the rows cluster_text prints are the cores; its lists are the tallies
        lines = text.split("\n")
        printed = {line.split("\t")[0] for line in lines if line.count("\t") == 3}
        cores = {g.seqs[i] for i in range(g.n) if x.core[a + i]}
        assert len(set(g.seqs)) == g.n and cores <= printed, k
        assert printed - cores <= {g.seqs[int(c)] for c in x.centers[c0:c0 + r["NCLUST"]]}, k       # (a centre that is halo)
        t = x.tallies[c0:c0 + r["NCLUST"]].astype(np.int64)
        ints = lambda key: [int(v) for v in [ln for ln in lines if ln.startswith(key)][0].split(": ")[1].split("=")[0].split("+") if v]
        assert t[:, 2].tolist() == ints("total Cluster Core Read Count") and t[:, 3].tolist() == ints("total Cluster Halo Read Count"), k
        shown = [ln for ln in lines if ln.startswith("Cluster: ")]
        assert len(shown) == int((t[:, 2] > 0).sum()), k
        for ln, row in zip(shown, t[t[:, 2] > 0]):
            assert [int(v) for v in ln.split("Elements: ")[1].split(" ")[0:3:2]] == row[:2].tolist(), k
        for c in range(r["NCLUST"]):
            assert t[c, 0] == int((r["cl"][1:] == c + 1).sum()) and (t[c, 2] > 0 or t[c, 1] == 0), k
        # the order: the members of each cluster together and in row order, the rows of no cluster last
        seg = x.order[a:b].astype(np.int64)
        lab = x.labels[seg]
        slot = np.where(lab >= 1, lab - 1, r["NCLUST"])
        assert sorted(seg.tolist()) == list(range(a, b)) and (np.diff(slot) >= 0).all() and (np.diff(seg)[np.diff(slot) == 0] > 0).all(), k


# ---------------------------------------------------------------- the writer
@pytest.mark.parametrize("name", WORLDS + ("hand",))
def test_writer_equals_write_clusters(worlds, name, golden, tmp_path, monkeypatch):  # noqa: F811
    w, ref, x = worlds[name]
    want = w.reference_files(str(tmp_path / "ref"), ref)
    if name != "hand":
        files = expected_files(golden["worlds"][name])
        assert all(files[k] == v for k, v in want.items()) and len(want) == 2 * len(w.sample_list)
    monkeypatch.setenv("MIRGE_AMD_TRF_SAMPLE_BLOCK_ROWS", "3")          # (runs of about three groups)
    for threads in ("1", "5", "16"):
        monkeypatch.setenv("MIRGE_AMD_TABLE_THREADS", threads)
        got = w.write(str(tmp_path / threads), x)
        for k in want:
            assert got[k] == want[k], (k, threads)
    if name == "hand":
        det = want["s0.fastq.potential_tRFs.clusters.detail"]
        assert "Number of Clusters: 2\n" in det and "=" in det and "N" in det and want["s2.fastq.tRFs.report.tsv"].count("\n") == 1
        assert "\tY:" in want["s0.fastq.tRFs.report.tsv"] and "pre_tA_trailer" not in want["s0.fastq.tRFs.report.tsv"]


def test_writer_raises_what_the_record_route_raises(tmp_path):
    w = hand_world()
    ref, x = w.reference(), w.arrays()
    # a selected name with "pre" in it whose key is a selected name without template in trnaStruDic
    w.names[4], w.names[0] = "pre_pre_tQ_trailer_x", "pre_tQ_trailer"
    w.pre = dict(w.pre, pre_pre_tQ_trailer_x=w.stru["tD"]["seq"], pre_tQ_trailer=w.stru["tA"]["seq"])
    ref = w.reference()
    with pytest.raises(KeyError) as e1:
        w.reference_files(str(tmp_path / "ref"), ref)
    with pytest.raises(KeyError) as e2:
        w.write(str(tmp_path / "new"), x)
    assert e1.value.args == e2.value.args == ("pre_tQ_trailer",) and os.listdir(str(tmp_path / "new")) == []
    # a tRF longer than the template it is compared with (the pairing quirk): detect_mismatch's IndexError
    w = hand_world()
    ref, x = w.reference(), w.arrays()
    w.stru = dict(w.stru, tE={"seq": w.stru["tE"]["seq"][:20]})
    with pytest.raises(IndexError):
        w.reference_files(str(tmp_path / "ref2"), ref)
    with pytest.raises(IndexError):
        w.write(str(tmp_path / "new2"), x)
    assert os.listdir(str(tmp_path / "new2")) == []


def test_writer_refuses_arrays_that_contradict_each_other(tmp_path):
    from mirge_amd._native import MirgeAmdError
    w = hand_world()
    x = w.arrays()
    for change in ("tally", "order", "label", "centre", "core"):
        y = types.SimpleNamespace(**{k: np.array(v) for k, v in vars(x).items()})
        if change == "tally":
            y.tallies[2, 2] += 1
        elif change == "order":
            a = int(w.off[3])
            y.order[[a, a + 1]] = y.order[[a + 1, a]]
        elif change == "label":
            y.labels[int(w.off[3]) + 2] = 3
        elif change == "centre":
            y.centers[int(y.cen_off[3])] = 4
        else:
            y.core[int(w.off[3])] = 1
        with pytest.raises(MirgeAmdError):
            w.write(str(tmp_path / change), y)


@pytest.mark.parametrize("world", WORLDS)
def test_write_trf_samples_arrays_with_device_labels_equals_the_reference(golden, world, tmp_path, monkeypatch):  # noqa: F811
    a = golden_arrays(golden, world, str(tmp_path / "libs"))
    monkeypatch.setattr(trf_samples, "cluster_text", None)       # (the route must not walk the groups in Python)
    monkeypatch.setattr(trf_samples, "peaks_results", None)
    timings = {}
    tdir = trf_samples.write_trf_samples_arrays(str(tmp_path), a.sample_list, a.et, a.st, a.rec, a.words, a.lens, a.nmask, a.quant,
                                                a.denom, a.tables, a.pre, model_groups, trf_samples.layout_peaks(model_label_peaks),
                                                timings=timings, device_labels=True)
    check_dir(golden["worlds"][world], tdir)
    assert {"groups_s", "reports_s", "peaks_s", "clusters_s"} <= set(timings)


def test_write_trf_samples_arrays_with_device_labels_on_the_hand_made_reads(tmp_path):
    """The world of tests/test_trf_groups.py: its empty leading block shifts the pairing, so a tRF of the 255-nt template is
    compared with a shorter one and the record route ends in detect_mismatch's IndexError.  The new route raises it too,
    before it writes either of its two files."""
    from tests.trf_peaks_model import model_peaks
    a = groups_hand_world()
    with pytest.raises(IndexError):
        trf_samples.write_trf_samples(str(tmp_path / "record"), a.sample_list, content_from(a), a.tables, a.pre, model_peaks)
    with pytest.raises(IndexError):
        trf_samples.write_trf_samples_arrays(str(tmp_path / "arrays"), a.sample_list, a.et, a.st, a.rec, a.words, a.lens, a.nmask,
                                             a.quant, a.denom, a.tables, a.pre, model_groups,
                                             trf_samples.layout_peaks(model_label_peaks), device_labels=True)
    left = sorted(os.listdir(str(tmp_path / "arrays" / "tRFs.samples.tmp")))
    assert left == sorted(s + x for s in a.sample_list for x in (".potential_tRFs.report", ".potential_tRFs.summary.report"))
    for fn in left:
        with open(str(tmp_path / "record" / "tRFs.samples.tmp" / fn)) as f1, open(str(tmp_path / "arrays" / "tRFs.samples.tmp" / fn)) as f2:
            assert f1.read() == f2.read(), fn


def test_a_run_without_any_group(tmp_path):
    from tests.trf_peaks_model import model_peaks
    a = groups_hand_world()
    a.quant[:] = 0
    want = trf_samples.write_trf_samples(str(tmp_path / "record"), a.sample_list, content_from(a), a.tables, a.pre, model_peaks)
    got = trf_samples.write_trf_samples_arrays(str(tmp_path / "arrays"), a.sample_list, a.et, a.st, a.rec, a.words, a.lens, a.nmask,
                                               a.quant, a.denom, a.tables, a.pre, model_groups,
                                               trf_samples.layout_peaks(model_label_peaks), device_labels=True)
    assert sorted(os.listdir(got)) == sorted(os.listdir(want)) and len(os.listdir(got)) == 4 * len(a.sample_list)
    for fn in os.listdir(want):
        with open(os.path.join(want, fn)) as f1, open(os.path.join(got, fn)) as f2:
            assert f1.read() == f2.read(), fn


# ---------------------------------------------------------------- repr(float)
def test_py3_float_repr(native_lib):
    buf = C.create_string_buffer(40)

    def native(v):
        assert native_lib.mrg_py3_float_repr(v, buf, 40) == 0
        return buf.value.decode()
    values = [0.0, -0.0, 1.0, 2.0, 10.0, 100.0, 123456789.0, 2.0 ** 53, 1e-5, 1e-4, 9.999e15, 1e16, 1.5e16, 1e22, 1e23, 5e-324,
              1.7976931348623157e308, 0.1, 0.3, 1 / 3.0, 2.5e-5, 0.00012345, float("inf"), -float("inf"), -17.125]
    acc = 0.0
    for k in range(1, 3000):
        acc += k / 1000.0
        values += [acc, k / 1000.0]
    rng = np.random.default_rng(23)
    values += rng.integers(0, 2 ** 63, 100_000, dtype=np.uint64).view(np.float64).tolist()      # any exponent
    values += (rng.random(20_000) * 10.0 ** rng.integers(-6, 18, 20_000)).tolist()
    for v in values:
        if v == v:
            assert native(v) == repr(v), v
    assert native(float("nan")) == "nan"
    assert native_lib.mrg_py3_float_repr(1.0, None, 40) < 0 and native_lib.mrg_py3_float_repr(1.0, buf, 8) < 0


# ---------------------------------------------------------------- C-ABI argument checks (no GPU needed)
def test_entry_points_refuse_bad_arguments(native_lib, tmp_path):
    L = native_lib
    x = C.c_void_p(8)   # (a non-null pointer, never dereferenced: every call below fails its checks first)
    off, bad_off, off1 = (C.c_uint32 * 3)(0, 2, 5), (C.c_uint32 * 3)(0, 4, 2), (C.c_uint32 * 3)(1, 2, 5)
    u32 = lambda *v: np.array(v, dtype=np.uint32)

    def assign(ctx=x, o=off, G=2, rho=x, rank=x, delta=x, nn=x, label=x, nclust=x, cap=5, cen_off=x, centers=x):
        return L.mrg_trf_assign(ctx, o, G, rho, rank, delta, nn, label, nclust, cap, cen_off, centers, None)
    assert assign(ctx=None) < 0 and b"null" in L.mrg_last_error()
    assert assign(o=None) < 0 and assign(G=0) < 0 and assign(nclust=None) < 0 and assign(cen_off=None) < 0
    assert assign(o=bad_off) < 0 and b"decrease" in L.mrg_last_error()
    assert assign(o=off1) < 0
    for k in ("rho", "rank", "delta", "nn", "label", "centers"):
        assert assign(**{k: None}) < 0 and b"null" in L.mrg_last_error(), k

    def halo(ctx=x, o=off, max_len=76, label=x, counts=x, stride=1, cen_off=u32(0, 1, 2), centers=u32(0, 1), bord_off=u32(0, 0, 0),
             bord=None, core=x, order=x, tallies=x):
        p = lambda v: v.ctypes.data if isinstance(v, np.ndarray) else v
        return L.mrg_trf_halo(ctx, o, 2, max_len, x, None, x, x, label, counts, stride, p(cen_off), p(centers), p(bord_off), bord,
                              core, order, tallies, None)
    assert halo(ctx=None) < 0 and b"null" in L.mrg_last_error()
    assert halo(o=None) < 0 and halo(o=bad_off) < 0 and halo(cen_off=None) < 0 and halo(bord_off=None) < 0
    assert halo(max_len=256) < 0 and b"255" in L.mrg_last_error()
    for k in ("label", "counts", "core", "order", "tallies"):
        assert halo(**{k: None}) < 0 and b"null" in L.mrg_last_error(), k
    assert halo(stride=0) < 0
    assert halo(cen_off=u32(1, 1, 2)) < 0 and halo(cen_off=u32(0, 2, 1)) < 0 and b"decrease" in L.mrg_last_error()
    assert halo(cen_off=u32(0, 3, 3), centers=u32(0, 1, 1)) < 0 and b"more centres" in L.mrg_last_error()
    assert halo(centers=u32(2, 1)) < 0 and b"none of its rows" in L.mrg_last_error()
    assert halo(centers=None) < 0
    assert halo(cen_off=u32(0, 2, 3), centers=u32(0, 1, 0)) < 0 and b"border slots" in L.mrg_last_error()
    assert halo(cen_off=u32(0, 2, 3), centers=u32(0, 1, 0), bord_off=u32(0, 3, 3), bord=None) < 0 and b"null" in L.mrg_last_error()

    paths = (C.c_char_p * 2)(os.fsencode(str(tmp_path / "a")), os.fsencode(str(tmp_path / "b")))
    names = (C.c_char_p * 2)(b"t", b"u")
    st = (C.c_int64 * 2)()

    def write(p=paths, S=1, codes=x, max_len=76, stride=5, n=5, o=off.__class__(0, 2, 5), G=2, names_=names, labels=x, status=st):
        return L.mrg_write_trf_cluster_reports(p, S, codes, None, max_len, stride, x, x, x, n, C.addressof(o) if o is not None else None,
                                               G, x, x, names_, names, names, names, labels, x, x, x, x, x, x, status)
    assert write(p=None) < 0 and b"null" in L.mrg_last_error()
    assert write(S=0) < 0 and write(status=None) < 0 and write(o=None) < 0 and write(codes=None) < 0 and write(labels=None) < 0
    assert write(names_=None) < 0 and b"group tables" in L.mrg_last_error()
    assert write(max_len=0) < 0 and write(max_len=256) < 0 and write(stride=4) < 0
    assert write(o=bad_off) < 0 and b"decrease" in L.mrg_last_error()
    assert write(o=off1) < 0 and write(n=4) < 0 and b"cover" in L.mrg_last_error()
    assert sorted(os.listdir(str(tmp_path))) == []
