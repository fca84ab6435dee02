"""The array route of tRFs.samples.tmp/ without a GPU: the numpy statement of the blocks (tests/trf_groups_model.py)
against the Python route of mirge_amd/trf_samples.py (sample_trf_dic -> sample_reports -> load_data_new -> Group ->
layout) on the golden worlds and a hand-made one; the native writer (mrg_write_trf_sample_reports) and
write_trf_samples_arrays against the reference's files; the RP100K text rule; argument checks of the C-ABI."""
import ctypes as C
import os
import types

import numpy as np
import pytest

from mirge_amd import pack, trf, trf_samples
from tests.test_trf_samples import WORLDS, check_dir, content_of, expected_files, golden, tables_of  # noqa: F401
from tests.trf_groups_model import model_groups, rp100k_text
from tests.trf_peaks_model import model_peaks


# ---------------------------------------------------------------- worlds as arrays
def arrays_of(names, aa_types, tables, pre, sample_list, denom, reads, quant, rows):
    """rows: (read index, entry, start, type index, kind) in the order of the tsv."""
    errors = {}
    for e, name in enumerate(names):
        try:
            pre[name] if "pre" in name else tables["trnaStruDic"][name]["seq"]
        except KeyError as err:
            errors[(e, "length")] = err
    et = types.SimpleNamespace(names=list(names), aa_types=list(aa_types), errors=errors)
    words, lens, nmask = pack.pack_reads(reads)
    rec = np.zeros((len(rows), 12), dtype=np.int32)
    for r, (ri, entry, start, ti, kind) in enumerate(rows):
        rec[r, :5] = (ri, entry, start, start + len(reads[ri]) - 1, ti)
        rec[r, 7] = kind
    return types.SimpleNamespace(et=et, st=trf.sample_tables(et, tables, pre), rec=rec, words=words, lens=lens, nmask=nmask,
                                 quant=np.array(quant, dtype=np.uint32).reshape(len(reads), -1), tables=tables, pre=pre,
                                 denom=np.array(denom, dtype=np.uint64), sample_list=list(sample_list), reads=list(reads))


def golden_arrays(golden, world, root):  # noqa: F811
    w = golden["worlds"][world]
    tables, pre = tables_of(golden, root)
    names = w["trf_names"]
    aa = [tables["trnaAAanticodonDic"][x]["aaType"] for x in names]
    rows = [(ri, ni, start, trf.TRF_TYPES.index(w["trf_types"][ti]), trf.KIND_ASSIGNED) for ri, ni, start, ti in w["trfContentDic"]]
    denom = [q["maturetrnaReads"] + q["pretrnaReads"] for q in w["quantStats"]]
    return arrays_of(names, aa, tables, pre, w["sample_list"], denom, [r[0] for r in w["reads"]], [r[1:] for r in w["reads"]],
                     rows)


def content_from(a):
    """The trfContentDic of the Python route for the arrays `a` (what trf.content_from_rows builds)."""
    out = {}
    for row in a.rec.tolist():
        if row[7] > trf.KIND_DELE:
            continue
        counts = [int(x) for x in a.quant[row[0]]]
        out[a.reads[row[0]]] = {"uid": "", "count": counts,
                                "RPM": [100000.0 * c / int(d) if d else 0.0 for c, d in zip(counts, a.denom)],
                                a.et.names[row[1]]: {"tRFType": trf.TRF_TYPES[row[4]], "start": row[2], "cigar": "undifined"}}
    return out


def python_route(a, content):
    """(report text, summary text) per sample, the groups, and the name each group is paired with."""
    stru, aa = a.tables["trnaStruDic"], a.tables["trnaAAanticodonDic"]
    sdic = trf_samples.sample_trf_dic(content, a.sample_list, stru, a.pre)
    files, groups, paired = [], [], []
    for s in a.sample_list:
        lines, summary = trf_samples.sample_reports(sdic[s], stru, aa, a.pre)
        files.append(("".join(lines), summary))
        blocks = trf_samples.load_data_new(lines)
        names = [line.split("\t")[0] for line in lines if "RP100K sum:" in line]
        paired += names[:len(blocks)]
        groups += [trf_samples.Group(rows) for rows in blocks]
    return files, groups, paired


def assert_model_equals_python(a, content):
    files, groups, paired = python_route(a, content)
    g = model_groups(a.st, a.rec, a.words, a.lens, a.nmask, a.quant, a.denom)
    assert g.filled and g.G == len(groups)
    assert [a.et.names[g.blocks[b, 1]] for b in g.groups[:, 1]] == paired
    if groups:
        off, codes, nmask, span, rpm, max_len = trf_samples.layout(groups)
        assert max_len == g.max_len and np.array_equal(off, g.off)
        assert np.array_equal(codes, g.codes) and np.array_equal(span, g.span)
        assert (nmask is None) == (g.nmask is None) and (nmask is None or np.array_equal(nmask, g.nmask))
        assert np.array_equal(rpm.view(np.uint64), g.rpm.view(np.uint64))
        for k, grp in enumerate(groups):
            a0, a1 = int(g.off[k]), int(g.off[k + 1])
            assert grp.counts == g.rows[a0:a1, 1].tolist()
            assert grp.types == [trf.TRF_TYPES[t] for t in g.rows[a0:a1, 2]]
    return g, files


def native_files(a, g, tdir):
    os.makedirs(tdir, exist_ok=True)
    trf_samples.write_trf_sample_reports(tdir, a.sample_list, a.st, a.et, g, a.rec, a.words, a.lens, a.nmask, a.quant, a.denom)
    out = []
    for s in a.sample_list:
        with open(os.path.join(tdir, s + ".potential_tRFs.report")) as f1, \
                open(os.path.join(tdir, s + ".potential_tRFs.summary.report")) as f2:
            out.append((f1.read(), f2.read()))
    return out


# ---------------------------------------------------------------- the model against the Python route
@pytest.mark.parametrize("world", WORLDS)
def test_model_equals_the_python_route_on_the_golden_worlds(golden, world, tmp_path):  # noqa: F811
    a = golden_arrays(golden, world, str(tmp_path / "libs"))
    g, _ = assert_model_equals_python(a, content_of(golden["worlds"][world]))
    if world == "large":      # an empty block, rows with N, one- and two-row blocks, blocks of 200+ rows
        sizes = set(g.blocks[:, 3].tolist())
        assert {0, 1, 2} <= sizes and max(sizes) >= 200 and g.has_n


def rand_seq(rng, n):
    return "".join("ACGT"[c] for c in rng.integers(0, 4, n))


def hand_world(long_template=255, missing=False):
    rng = np.random.default_rng(5)
    names = ["tA", "tB", "tA", "pre_tC_trailer", "tE", "tLong", "tZ", "tMissing"]
    stru = {"tA": rand_seq(rng, 100), "tB": rand_seq(rng, 100), "tE": rand_seq(rng, 20), "tLong": rand_seq(rng, long_template),
            "tZ": rand_seq(rng, 76)}
    pre = {"pre_tC_trailer": rand_seq(rng, 40)}
    aa = {"tA": "Ala", "tB": "Gly", "pre_tC_trailer": "Cys", "tE": "Glu", "tLong": "Leu", "tZ": "Ala", "tMissing": "Met"}
    tables = {"trnaStruDic": {k: {"seq": v} for k, v in stru.items()},
              "trnaAAanticodonDic": {k: {"aaType": v, "anticodon": "XXX"} for k, v in aa.items()}}
    x = "ACGGTCATTGCAATCGGTAC"
    reads, quant, rows = [], [], []

    def add(read, counts, entry, start, ti=6, kind=trf.KIND_ASSIGNED):
        reads.append(read)
        quant.append(counts)
        rows.append((len(reads) - 1, entry, start, ti, kind))
    # string order at equal count and start: a proper prefix first, N between G and T; two entries of one name
    for k, read in enumerate((x + "G", x, x + "N", x + "T", x + "GA")):
        add(read, [5, 5, 0], 0 if k % 2 else 2, 10, 5)
    add(rand_seq(rng, 30), [5, 0, 0], 0, 1, 3)                 # (a count of 0 in one sample; start <= 2: 5')
    add(rand_seq(rng, 30), [9, 2, 0], 2, 70, 5)                # (ends at the template's end: 3')
    add(rand_seq(rng, 25), [4, 1, 0], 1, 40)                   # tB and tZ: equal read_sum in sample 0
    add(rand_seq(rng, 22), [3, 1, 0], 1, 3)
    add(rand_seq(rng, 24), [7, 3, 0], 6, 50)
    add(rand_seq(rng, 21), [50, 0, 0], 4, 0)                   # tE: its one item overhangs, and it leads sample 0
    add(rand_seq(rng, 18) + "TTT", [6, 6, 0], 3, 19, 0)        # the trailer: start + len == template length
    add(rand_seq(rng, 19) + "TTT", [2, 8, 0], 3, 19, 0)        # ... and one more: overhangs
    for k, start in enumerate((25, 31, 32, 33, 63, 64, 65, long_template - 20, long_template - 19)):
        add(rand_seq(rng, 19) + ("N" if k == 2 else "A"), [k + 1, 2 * k + 1, 0], 5, start)
    add(rand_seq(rng, 20), [4, 4, 4], 0, 0, 6, trf.KIND_NONE)  # no candidate: no item (and sample 2 stays empty)
    if missing:
        add(rand_seq(rng, 20), [0, 3, 0], 7, 0)
        add(rand_seq(rng, 20), [1, 0, 0], 7, 0)
    return arrays_of(names, [aa[n] for n in names], tables, pre, ["s0.fastq", "s1.fastq", "s2.fastq"], [1000, 0, 500], reads,
                     quant, rows)


def test_hand_made_world():
    a = hand_world()
    g, files = assert_model_equals_python(a, content_from(a))
    names = [a.et.names[e] for e in g.blocks[:, 1]]
    s0 = [n for n, s in zip(names, g.blocks[:, 0]) if s == 0]
    assert s0[0] == "tE" and g.blocks[0, 3] == 0 and g.groups[0].tolist() == [1, 0]      # the pairing shifts
    assert s0.index("tZ") + 1 == s0.index("tB") and g.block_sums[s0.index("tZ")] == g.block_sums[s0.index("tB")] == 7
    assert sorted(set(g.blocks[:, 0].tolist())) == [0, 1] and files[2] == ("", "amino acid\tCounts\tRP100K\tUnique reads\n")
    ta = int(np.nonzero((g.blocks[:, 0] == 0) & (np.array(names) == "tA"))[0][0])
    first = int(g.blocks[ta, 2])
    order = [a.reads[a.rec[r, 0]][20:] for r in g.rows[first + 1:first + 6, 0]]
    assert order == ["T", "N", "GA", "G", ""] and g.blocks[ta, 1] == 0
    first1 = int(g.blocks[np.nonzero(g.blocks[:, 0] == 1)[0][0], 2])
    assert g.max_len == 255 and (g.rpm[first1:] == 0.0).all() and (g.rpm[:first1] > 0.0).all()   # denom == 0 in sample 1
    tc = names.index("pre_tC_trailer")
    assert g.blocks[tc, 3] == 1 and g.block_sums[tc] == 8


def test_hand_made_world_through_the_writer(tmp_path, monkeypatch):
    a = hand_world()
    g, files = assert_model_equals_python(a, content_from(a))
    monkeypatch.setenv("MIRGE_AMD_TRF_SAMPLE_BLOCK_ROWS", "3")
    for threads in ("1", "5"):
        monkeypatch.setenv("MIRGE_AMD_TABLE_THREADS", threads)
        assert native_files(a, g, str(tmp_path / threads)) == files


def test_template_of_256_nt_and_entry_without_template(tmp_path):
    a = hand_world(long_template=256)
    with pytest.raises(ValueError) as e1:
        trf_samples.layout(python_route(a, content_from(a))[1])
    backend = trf_samples.layout_peaks(model_peaks)
    with pytest.raises(ValueError) as e2:
        trf_samples.write_trf_samples_arrays(str(tmp_path), a.sample_list, a.et, a.st, a.rec, a.words, a.lens, a.nmask, a.quant,
                                             a.denom, a.tables, a.pre, model_groups, backend)
    assert str(e1.value) == str(e2.value) and "256" in str(e2.value)
    a = hand_world(missing=True)
    with pytest.raises(KeyError) as k1:
        python_route(a, content_from(a))
    with pytest.raises(KeyError) as k2:
        trf_samples.write_trf_samples_arrays(str(tmp_path / "x"), a.sample_list, a.et, a.st, a.rec, a.words, a.lens, a.nmask,
                                             a.quant, a.denom, a.tables, a.pre, model_groups, backend)
    assert k1.value.args == k2.value.args == ("tMissing",) and not os.path.exists(str(tmp_path / "x"))


# ---------------------------------------------------------------- the writer, write_trf_samples_arrays
@pytest.mark.parametrize("world", WORLDS)
def test_writer_equals_the_reference_files(golden, world, tmp_path, monkeypatch):  # noqa: F811
    w = golden["worlds"][world]
    a = golden_arrays(golden, world, str(tmp_path / "libs"))
    g = model_groups(a.st, a.rec, a.words, a.lens, a.nmask, a.quant, a.denom)
    want = expected_files(w)
    monkeypatch.setenv("MIRGE_AMD_TRF_SAMPLE_BLOCK_ROWS", "3")
    for threads in ("1", "5", "16"):
        monkeypatch.setenv("MIRGE_AMD_TABLE_THREADS", threads)
        got = native_files(a, g, str(tmp_path / threads))
        for s, (report, summary) in zip(a.sample_list, got):
            assert report == want[s + ".potential_tRFs.report"], (s, threads)
            assert summary == want[s + ".potential_tRFs.summary.report"], (s, threads)


@pytest.mark.parametrize("world", WORLDS)
def test_write_trf_samples_arrays_equals_the_reference(golden, world, tmp_path):  # noqa: F811
    a = golden_arrays(golden, world, str(tmp_path / "libs"))
    timings = {}
    tdir = trf_samples.write_trf_samples_arrays(str(tmp_path), a.sample_list, a.et, a.st, a.rec, a.words, a.lens, a.nmask,
                                                a.quant, a.denom, a.tables, a.pre, model_groups,
                                                trf_samples.layout_peaks(model_peaks), timings=timings)
    check_dir(golden["worlds"][world], tdir)
    assert {"groups_s", "reports_s", "peaks_s", "clusters_s"} <= set(timings)


def test_writer_refuses_null_and_inconsistent_arguments(native_lib, tmp_path):
    L = native_lib
    a = hand_world()
    g = model_groups(a.st, a.rec, a.words, a.lens, a.nmask, a.quant, a.denom)
    x = C.c_void_p(8)
    paths = (C.c_char_p * 2)(os.fsencode(str(tmp_path / "a")), os.fsencode(str(tmp_path / "b")))
    names = (C.c_char_p * 1)(b"t")
    assert L.mrg_write_trf_sample_reports(None, 1, x, x, 1, 0, x, None, 0, x, x, 0, x, names, names, names, 1, 1, x, x, 0, x, 0) < 0
    assert b"null" in L.mrg_last_error()
    assert L.mrg_write_trf_sample_reports(paths, 1, None, x, 1, 0, x, None, 0, x, x, 0, x, names, names, names, 1, 1, x, x, 0, x, 0) < 0
    assert L.mrg_write_trf_sample_reports(paths, 1, x, None, 1, 0, x, None, 0, x, x, 5, x, names, names, names, 1, 1, x, x, 0, x, 0) < 0
    assert L.mrg_write_trf_sample_reports(paths, 1, x, x, 3, 0, x, None, 0, x, x, 0, x, names, names, names, 1, 1, x, x, 0, x, 0) < 0
    assert b"words_per_read" in L.mrg_last_error()
    from mirge_amd._native import MirgeAmdError
    for change in ("sum", "rows", "order", "entry"):
        h = types.SimpleNamespace(blocks=g.blocks.copy(), block_sums=g.block_sums.copy(), rows=g.rows.copy())
        if change == "sum":
            h.block_sums[1] += 1
        elif change == "rows":
            h.rows = h.rows[:-1]
        elif change == "order":
            h.blocks[[0, -1]] = h.blocks[[-1, 0]]
        else:
            h.blocks[0, 1] = 99
        with pytest.raises(MirgeAmdError):
            trf_samples.write_trf_sample_reports(str(tmp_path), a.sample_list, a.st, a.et, h, a.rec, a.words, a.lens, a.nmask,
                                                 a.quant, a.denom)


# ---------------------------------------------------------------- the RP100K the peaks see
def test_rp100k_text_value(native_lib):
    f = native_lib.mrg_trf_rp100k_text
    pairs = [(c, 1_600_000) for c in (1, 3, 5)] + [(c, 200_000_000) for c in (125, 375)]     # exact ties
    for c, d in pairs:
        assert (100000.0 * c / d * 1000) % 1 == 0.5
    pairs += [(7, 7), (1, 1), (2 ** 40 - 1, 2 ** 40 - 1), (0, 5), (3, 0), (0, 0), (1, 2 ** 40 - 1), (1, 3), (2, 3)]
    rng = np.random.default_rng(11)
    d = rng.integers(1, 2 ** 40, 100_000)
    c = (rng.random(100_000) * (d + 1)).astype(np.int64).clip(0, d)
    small = rng.integers(1, 5000, 20_000)
    pairs += list(zip(c.tolist(), d.tolist())) + list(zip(rng.integers(0, 5000, 20_000).clip(0, small).tolist(), small.tolist()))
    for c, d in pairs:
        got, want = f(c, d), rp100k_text(c, d)
        assert got == want and np.float64(got).view(np.uint64) == np.float64(want).view(np.uint64), (c, d)


# ---------------------------------------------------------------- C-ABI argument checks (no GPU needed)
def test_device_entry_points_refuse_bad_arguments(native_lib):
    L = native_lib
    x = C.c_void_p(8)   # (a non-null pointer, never dereferenced: every call below fails its checks first)
    counts = (C.c_uint64 * 8)()
    denom = (C.c_uint64 * 2)(10, 10)
    good = np.array([[0, 30, 0, 0], [1, -1, 3, 0]], dtype=np.int32)

    def call(ctx=x, W=1, stride=10, n=10, S=2, k=5, den=denom, entries=good, names=2, cnt=counts):
        return L.mrg_trf_sample_groups(ctx, x, W, stride, x, None, n, x, S, x, k, den, entries.ctypes.data, entries.shape[0],
                                       names, 0, 0, None, None, None, None, None, None, None, None, None, cnt, None, None)
    assert call(ctx=None) < 0 and b"null" in L.mrg_last_error()
    assert call(cnt=None) < 0 and call(den=None) < 0 and call(S=0) < 0
    assert call(W=3) < 0 and b"words_per_read" in L.mrg_last_error()
    assert call(stride=5) < 0
    assert call(k=2 ** 31, S=2) < 0 and b"2^31" in L.mrg_last_error()
    assert call(k=2 ** 30, S=2) < 0 and b"2^31" in L.mrg_last_error()      # (2^31 pairs: a row number would not fit)
    assert call(names=2 ** 21 + 1) < 0 and b"cells" in L.mrg_last_error()
    for bad in ([[2, 30, 0, 0]], [[-1, 30, 0, 0]], [[0, -2, 0, 0]]):
        assert call(entries=np.array(bad, dtype=np.int32)) < 0 and b"entry 0" in L.mrg_last_error()
    off, bad_off, off1 = (C.c_uint32 * 3)(0, 2, 5), (C.c_uint32 * 3)(0, 4, 2), (C.c_uint32 * 3)(1, 2, 5)
    assert L.mrg_trf_rank(None, off, 2, x, x, None) < 0 and b"null" in L.mrg_last_error()
    assert L.mrg_trf_rank(x, None, 2, x, x, None) < 0 and L.mrg_trf_rank(x, off, 0, x, x, None) < 0
    assert L.mrg_trf_rank(x, bad_off, 2, x, x, None) < 0 and L.mrg_trf_rank(x, off1, 2, x, x, None) < 0
    assert L.mrg_trf_rank(x, off, 2, None, x, None) < 0 and L.mrg_trf_rank(x, off, 2, x, None, None) < 0
