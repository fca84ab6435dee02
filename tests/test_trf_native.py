"""The array route of `-trf` on the CPU: trf.entry_tables against the per-read expressions of
collect_trf_content / write_trf_tables, and the native writer (mrg_write_trf_tables, with trf.row_order
and trf.raise_unresolved in front of it) against trf.write_trf_tables, fed with rows that
tests/trf_rows_model.py derives from the functions of trf.py.  The kernels that produce those rows on
the GPU are tested in tests/test_gpu_trf_tables.py."""
import copy
import json
import os

import numpy as np
import pytest

from mirge_amd import columnar, pack, trf
from tests import trf_rows_model as model
from tests.conftest import ROOT
from tests.test_trf import FILES, check_files, oracle_lister, write_world


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "trf.json")) as fh:
        return json.load(fh)


def golden_world(golden, root):
    write_world(golden, root)
    tables = trf.load_trf_tables(root, "human")
    pre = dict(zip(*golden["libraries"]["pre_trna"]))
    et = trf.entry_tables(golden["libraries"]["mature_trna"][0], golden["libraries"]["pre_trna"][0], tables, pre)
    return tables, pre, et


def unpack_dashed(et, t):
    first, last, n, word = (int(x) for x in et.clusters[t, :4])
    out = []
    for i in range(n):
        w, sh = word + (i >> 5), 2 * (i & 31)
        code, flag = (int(et.words[w]) >> sh) & 3, (int(et.plane[w]) >> sh) & 3
        out.append("-" if flag & 2 else ("N" if code == 0 else "?") if flag & 1 else "ACGT"[code])
    return "".join(out)


def check_entry_tables(et, mature_names, pre_names, tables, pre):
    """Every column of the tables against the expression the per-read code evaluates."""
    stru, aa, dup = tables["trnaStruDic"], tables["trnaAAanticodonDic"], tables["duptRNA2UniqueDic"]
    names = list(mature_names) + list(pre_names)
    assert et.names == names and et.n_mature == len(mature_names)
    reps = [dup.get(x, x) for x in names]
    order = sorted(set(reps))
    for e, name in enumerate(names):
        tlen, n_type, anticodon, flags, rank, rep, first, count = (int(x) for x in et.desc[e])
        try:
            assert tlen == (len(pre[name]) if "pre" in name else len(stru[name]["seq"]))
        except KeyError as err:
            assert tlen == -1 and repr(et.errors[(e, "length")]) == repr(err)
        assert bool(flags & 1) == ("pre_" in name)
        try:
            trf.trfTypes("ACGT", name, 1, stru, pre)
            assert not flags & 2
            if not flags & 1:
                assert (n_type, anticodon) == (len(stru[name]["seq"]), stru[name]["anticodonStart"] - 1)
        except KeyError as err:
            assert flags & 2 and repr(et.errors[(e, "type")]) == repr(err)
        assert order[rank] == reps[e] == et.rep_names[e]
        lib = range(len(mature_names)) if e < len(mature_names) else range(len(mature_names), len(names))
        assert rep == next((x for x in lib if names[x] == reps[e]), -1)
        if name in aa:
            assert (et.aa_types[e], et.anticodons[e]) == (aa[name]["aaType"], aa[name]["anticodon"])
        else:
            assert et.aa_types[e] is None and isinstance(et.errors[(e, "aa")], KeyError)
        assert et.rep_aa_missing[e] == (reps[e] not in aa)
        want = list(tables["tRNAtrfDic"].get(name, {}).items())
        assert count == len(want)
        for t, (dashed, cname) in zip(range(first, first + count), want):
            assert et.cluster_names[t] == cname and et.dashed[t] == dashed
            assert (int(et.clusters[t, 0]), int(et.clusters[t, 1])) == trf.coordinate(dashed)
            assert int(et.clusters[t, 2]) == len(dashed) and unpack_dashed(et, t) == dashed
            m = int(et.clusters[t, 5])
            if cname in tables["trfMergedNameDic"]:
                assert tables["trfMergedList"][m] == tables["trfMergedNameDic"][cname]
            else:
                assert m == -1 and isinstance(et.errors[("cluster", t)], KeyError)
    # cluster name ranks order as the names do
    for a in range(len(et.cluster_names)):
        for b in range(len(et.cluster_names)):
            assert (et.clusters[a, 4] < et.clusters[b, 4]) == (et.cluster_names[a] < et.cluster_names[b])


def test_entry_tables_on_the_golden_world(golden, tmp_path):
    tables, pre, et = golden_world(golden, str(tmp_path))
    check_entry_tables(et, golden["libraries"]["mature_trna"][0], golden["libraries"]["pre_trna"][0], tables, pre)
    assert et.clusters.shape[0] > 10 and not et.errors
    # the golden has a duplicate pair in both libraries (every predefined string of it is as long as its tRNA: the
    # shorter one is in the hand-made world below)
    assert sum(int(et.desc[e, 5]) != e for e in range(len(et.names))) == 2


# ---- a hand-made world: every failure status, a tRNA without predefined tRFs, a tie in distance, a short predefined string
T1 = "GCATTGGTGGTTCAGTGGTAGAATTCTCGCCTGCCACGCGGGAGGCCCGGGTTCGATTCCCGGCCAATGCACCAGCA"   # 76 nt
T2 = "GGGGGTATAGCTCAGTGGTAGAGCGCGTGCTTAGCATGCACGAGGTCCTGGGTTCGATCCCCAGTACCTCCACCAA"
PRE1 = "GTTCGAATCCGGGTGCATTGCAACTGTTTTTGCA"
STRU = "(" * 33 + "XXX" + ")" * 40


T3 = "".join(__import__("random").Random(5).choice("ACGT") for _ in range(76))
T4 = "".join(__import__("random").Random(6).choice("ACGT") for _ in range(76))


def hand_world():
    mature = ["tRNA-b", "tRNA-a", "tRNA-c", "tRNA-nostru", "tRNA-noaa", "tRNA-dupgone", "tRNA-notrf", "premature-x", "tRNA-und"]
    seqs = [T2, T2, T1, T1[::-1], T2[::-1], T4, T2[7:] + "CCATGCA", T3, T2[2:] + "TC"]
    pre = ["pre_a_trailer", "pre_b_trailer", "nopre-trailer"]
    pre_seq = [PRE1, PRE1, PRE1[::-1]]
    stru = {n: {"seq": s, "stru": STRU, "anticodonStart": 34, "anticodonEnd": 36}
            for n, s in zip(mature, seqs) if n not in ("tRNA-nostru", "premature-x")}
    aa = {n: {"aaType": "Gly", "anticodon": "GCC"} for n in mature + pre if n != "tRNA-noaa"}
    aa["tRNA-und"] = {"aaType": "Und", "anticodon": "NNN"}
    aa["pre_b_trailer"] = {"aaType": "Und", "anticodon": "NNN"}
    dup = {"tRNA-b": "tRNA-a", "tRNA-dupgone": "tRNA-gone", "pre_b_trailer": "pre_a_trailer"}
    clusters = {
        "tRNA-a": {trf.add_dash_new(T2[:30], 76, 1, 30): "tRNA-a_Cluster2", trf.add_dash_new(T2[2:32], 76, 3, 32): "tRNA-a_Cluster1",
                   trf.add_dash_new(T2[50:], 76, 51, 76): "tRNA-a_Cluster3"},
        "tRNA-c": {trf.add_dash_new(T1[:19], 19, 1, 19): "tRNA-c_Cluster1"},              # shorter than its tRNA
        "tRNA-und": {trf.add_dash_new("ACNTG" + T2[7:25], 76, 3, 25): "tRNA-und_Cluster1"},   # N on the predefined tRF
        "pre_a_trailer": {trf.add_dash_new(PRE1[:20], len(PRE1), 1, 20): "pre_a_trailer_Cluster1"},
        "tRNA-noaa": {trf.add_dash_new(T2[::-1][:30], 76, 1, 30): "tRNA-noaa_Cluster1"},
    }
    merged_name = {"tRNA-a_Cluster1": "a_5p", "tRNA-a_Cluster2": "a_5p", "tRNA-c_Cluster1": "c_5p",
                   "pre_a_trailer_Cluster1": "a_trailer", "tRNA-und_Cluster1": "und_5p",
                   "tRNA-noaa_Cluster1": "noaa_5p"}   # (tRNA-a_Cluster3: missing)
    tables = {"trnaStruDic": stru, "trnaAAanticodonDic": aa, "duptRNA2UniqueDic": dup, "tRNAtrfDic": clusters,
              "trfMergedNameDic": merged_name, "trfMergedList": ["a_5p", "c_5p", "a_trailer", "und_5p", "noaa_5p"]}
    libs = {"mature_trna": (mature, seqs), "pre_trna": (pre, pre_seq)}
    return libs, tables, dict(zip(pre, pre_seq))


def test_entry_tables_keep_every_failure_until_a_read_reaches_it():
    libs, tables, pre = hand_world()
    mature, pre_names = libs["mature_trna"][0], libs["pre_trna"][0]
    et = trf.entry_tables(mature, pre_names, tables, pre)
    check_entry_tables(et, mature, pre_names, tables, pre)
    e = {n: i for i, n in enumerate(et.names)}
    assert set(et.errors) == {(e["tRNA-nostru"], "type"), (e["tRNA-nostru"], "length"), (e["tRNA-noaa"], "aa"),
                              (e["premature-x"], "type"), (e["premature-x"], "length"), (e["nopre-trailer"], "type"),
                              ("cluster", 2)}   # ("pre" in "nopre-trailer": its template is its pre-tRNA sequence)
    assert et.desc[e["tRNA-dupgone"], 5] == -1 and et.rep_aa_missing[e["tRNA-dupgone"]]
    assert et.desc[e["tRNA-b"], 5] == e["tRNA-a"] and et.desc[e["pre_b_trailer"], 5] == e["pre_a_trailer"]
    assert et.desc[e["tRNA-notrf"], 7] == 0 and et.desc[e["tRNA-a"], 7] == 3
    assert int(et.clusters[int(et.desc[e["tRNA-c"], 6]), 2]) == 19 < int(et.desc[e["tRNA-c"], 0])
    # "premature-x": "pre" in the name but not "pre_" -- typed from trnaStruDic, its template from the pre-tRNA sequences
    assert not et.desc[e["premature-x"], 3] & 1


def write_both(native_lib, tmp_path, sample_list, quant_stats, tables, pre, et, mature, trailer, quant, lister, threads=None,
               block_rows=None, monkeypatch=None):
    """The Python route and the native writer on the same reads -> (python dir, native dir, content, rec in tsv order)."""
    py_dir, nat_dir = tmp_path / "python", tmp_path / ("native_%s" % threads)
    py_dir.mkdir(exist_ok=True)
    nat_dir.mkdir(exist_ok=True)
    reads = list(mature) + list(trailer)
    sd = model.seq_dic(mature, trailer, quant)
    content = {}
    trf.collect_trf_content(content, sd, sample_list, tables["trnaStruDic"], pre, lister)
    log_dic = {"quantStats": copy.deepcopy(quant_stats)}
    trf.write_trf_tables(str(py_dir), sample_list, log_dic, content, tables, pre)
    rec, hits = model.rows(et, tables, pre, mature, trailer, lister)
    words, lens, nmask = pack.pack_reads(reads)
    if monkeypatch is not None:
        if threads is not None:
            monkeypatch.setenv("MIRGE_AMD_TABLE_THREADS", str(threads))
        if block_rows is not None:
            monkeypatch.setenv("MIRGE_AMD_TRF_BLOCK_ROWS", str(block_rows))
    t_rec, n_rows = columnar.write_trf_tables(str(nat_dir), sample_list, log_dic, words, lens, nmask,
                                              np.array(quant, dtype=np.uint32), rec, hits, len(mature), et)
    assert n_rows == len(content)
    return py_dir, nat_dir, content, t_rec


def same_files(a, b):
    for fn in FILES:
        assert open(os.path.join(str(a), fn), "rb").read() == open(os.path.join(str(b), fn), "rb").read(), fn


@pytest.mark.parametrize("threads", [1, 5, 16])
def test_native_writer_on_the_golden_reads(golden, native_lib, oracle_lib, tmp_path, monkeypatch, threads):
    tables, pre, et = golden_world(golden, str(tmp_path / "libs"))
    sd = golden["state"]["seqDic"]
    mature = [s for s, r in sd.items() if r["annot"][3] != ""]
    trailer = [s for s, r in sd.items() if r["annot"][4] != ""]
    assert (len(mature), len(trailer)) == (173, 74)
    quant = [sd[s]["quant"] for s in mature + trailer]
    py_dir, nat_dir, content, t_rec = write_both(native_lib, tmp_path, golden["sample_list"], golden["state"]["quantStats"],
                                                 tables, pre, et, mature, trailer, quant, oracle_lister(golden), threads, 20,
                                                 monkeypatch)
    same_files(py_dir, nat_dir)
    check_files(golden, nat_dir)
    assert sum(int(r[9]) == 2 for r in t_rec) == 57
    # the adapter leaves what write_trf_tables leaves
    reads = mature + trailer
    seqs = [reads[i] for i in t_rec[:, 0]]
    denom = [q["maturetrnaReads"] + q["pretrnaReads"] for q in golden["state"]["quantStats"]]
    got = trf.content_from_rows(et, t_rec, seqs, np.array(quant)[t_rec[:, 0]], denom)
    assert got == content and list(got) == list(content)


def test_native_writer_edges(native_lib, tmp_path, monkeypatch):
    """Zero-denominator RP100K, a sample with count 0, a read with N (uid `.`), "Und" amino acids, a tie in distance, a
    predefined string shorter than the tRNA, Undef / Dele rows, a trailer group order that differs from the array order."""
    libs, tables, pre = hand_world()
    et = trf.entry_tables(libs["mature_trna"][0], libs["pre_trna"][0], tables, pre)
    mature = [T2[:30], T2[1:31], T2[1:20] + "N" + T2[21:31], T1[:21], T1[:25], T1[10:40], T2[7:] + "CCATGCA", T2[2:27],
              (T2[2:] + "TC")[-30:], T2[20:50]]
    trailer = [PRE1[:12] + "TTT", PRE1[:20] + "TTTT", PRE1[:12] + "TTTTT", PRE1[:20] + "TTT", "ACGGTCAGGTCA" + "TTT"]
    quant = [[k % 3, (k * 7) % 5] for k in range(len(mature) + len(trailer))]
    stats = [{"maturetrnaReads": 40, "pretrnaReads": 3}, {"maturetrnaReads": 0, "pretrnaReads": 0}]
    lister = model.brute_lister(libs)
    py_dir, nat_dir, content, t_rec = write_both(native_lib, tmp_path, ["a.fastq", "b.fastq"], stats, tables, pre, et, mature,
                                                 trailer, quant, lister, 3, 4, monkeypatch)
    same_files(py_dir, nat_dir)
    tsv = open(os.path.join(str(nat_dir), FILES[0])).read().split("\n")
    assert len(tsv) == len(mature) + len(trailer) - 1 + 2     # (the last trailer read has no candidate and is dropped)
    assert any(line.split("\t")[1] == "." for line in tsv[1:-1])
    assert all(line.split("\t")[3].endswith(",0.000") for line in tsv[1:-1])
    kinds = set(int(x) for x in t_rec[:, 7])
    assert kinds == {trf.KIND_ASSIGNED, trf.KIND_UNDEF, trf.KIND_DELE, trf.KIND_NONE}
    # the two stripped sequences interleave in array order: the rows are grouped by first appearance
    n2 = len(mature)
    assert [int(x) - n2 for x in t_rec[n2:, 0]] == [0, 2, 1, 3, 4]
    # the tie: tRNA-a_Cluster1 and _Cluster2 are equally far from T2[1:31]; the name decides
    row = next(r for r in t_rec if int(r[0]) == 1)
    assert et.cluster_names[int(row[5])] == "tRNA-a_Cluster1" and int(row[6]) == 2


def test_unresolvable_rows_raise_the_python_routes_exception(native_lib, tmp_path):
    libs, tables, pre = hand_world()
    et = trf.entry_tables(libs["mature_trna"][0], libs["pre_trna"][0], tables, pre)
    lister = model.brute_lister(libs)
    seqs = dict(zip(*libs["mature_trna"]))
    cases = [seqs["tRNA-noaa"][:25],            # a hit without amino acid
             seqs["tRNA-dupgone"][-30:],        # its de-duplicated name is no entry
             T2[50:76]]                         # assigned to a predefined tRF without merged entity
    for read in cases:
        sd = model.seq_dic([read], [], [[1]])
        content = {}
        trf.collect_trf_content(content, sd, ["s"], tables["trnaStruDic"], pre, lister)
        with pytest.raises(KeyError) as want:
            trf.write_trf_tables(str(tmp_path), ["s"], {"quantStats": [{"maturetrnaReads": 1, "pretrnaReads": 0}]}, content,
                                 tables, pre)
        rec, hits = model.rows(et, tables, pre, [read], [], lister)
        words, lens, nmask = pack.pack_reads([read])
        with pytest.raises(KeyError) as got:
            columnar.write_trf_tables(str(tmp_path), ["s"], {"quantStats": [{"maturetrnaReads": 1, "pretrnaReads": 0}]}, words,
                                      lens, nmask, np.array([[1]], dtype=np.uint32), rec, hits, 1, et)
        assert repr(got.value) == repr(want.value), read
    # a hit on an entry trfTypes cannot type: collect_trf_content raises; the row's hit says so
    read = seqs["tRNA-nostru"][3:30]
    with pytest.raises(KeyError) as want:
        trf.collect_trf_content({}, model.seq_dic([read], [], [[1]]), ["s"], tables["trnaStruDic"], pre, lister)
    e = et.names.index("tRNA-nostru")
    rec = np.zeros((1, 12), dtype=np.int32)
    rec[0, [1, 7, 9]] = (-1, trf.KIND_UNRESOLVABLE, 1)
    hits = np.array([[e, 3, 29, trf.TYPE_UNRESOLVABLE]], dtype=np.int32)
    with pytest.raises(KeyError) as got:
        trf.raise_unresolved(et, rec, hits)
    assert repr(got.value) == repr(want.value)
    # reads that reach none of these entries pass
    rec, hits = model.rows(et, tables, pre, [T2[:30]], [PRE1[:12] + "TTT"], lister)
    trf.raise_unresolved(et, rec, hits)
