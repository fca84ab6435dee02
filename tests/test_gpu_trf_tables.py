"""GPU (-m gpu): mrg_trf_classify (csrc/trf_tables.hip strung together in capi.hip) against the functions of
mirge_amd.trf through tests/trf_rows_model.py; then Engine.trf_classify + columnar.write_trf_tables and
`annotate -trf` with and without --trf-host.  Everything is compared for equality; there is no tolerance anywhere.

The direct calls put GUARD rows of a byte pattern behind the capacity of both output buffers, which must come back
untouched.  Libraries are tiny: the model lists by exhaustive comparison."""
import copy
import ctypes as C
import json
import os

import numpy as np
import pytest

from mirge_amd import pack, trf
from tests import trf_rows_model as model
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu

GUARD = 16
PAT = 0xA5
STRU = "(" * 33 + "XXX" + ")" * 40       # anticodonStart 34: trfTypes' anticodon = 33


def rnd_seq(rng, n, alphabet="ACGT"):
    return "".join(alphabet[int(x)] for x in rng.integers(0, len(alphabet), n))


class World:
    """Two tRNA libraries resident on the GPU, their tables and the model's lister."""

    def __init__(self, libs, tables, pre=None):
        import torch
        from mirge_amd.engine import Engine
        from mirge_amd.index import FmIndex
        self.torch = torch
        self.libs, self.tables = libs, tables
        self.pre = dict(zip(*libs["pre_trna"])) if pre is None else pre
        self.eng = Engine(0)
        for key in ("mature_trna", "pre_trna"):
            self.eng.add_library(key, FmIndex.build(*libs[key]))
        self.et = trf.entry_tables(libs["mature_trna"][0], libs["pre_trna"][0], tables, self.pre)
        self.lister = model.brute_lister(libs)
        self._cache = {}

    def up(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a)).to(self.eng.device)

    def call(self, words, lens, nmask, pass_id, cap_rows=None, cap_hits=None, pad=0):
        """mrg_trf_classify directly -> (rec, hits, n2, n3, kept) of what lies below the capacities (default: everything);
        the guards behind them are checked.  pad: columns of junk behind the reads (stride = n + pad)."""
        W, n = words.shape
        if pad:
            junk = np.full((W, pad), 0xDEADBEEFDEADBEEF, dtype=np.uint64)
            words = np.concatenate([words, junk], axis=1)
            nmask = None if nmask is None else np.concatenate([nmask, junk], axis=1)
        d_words = self.up(words.view(np.int64))
        d_nmask = None if nmask is None else self.up(nmask.view(np.int64))
        d_lens, d_pass = self.up(np.asarray(lens, dtype=np.uint8)), self.up(np.asarray(pass_id, dtype=np.int8))
        et, eng = self.et, self.eng
        desc, clusters = np.ascontiguousarray(et.desc), np.ascontiguousarray(et.clusters)
        counts = (C.c_uint64 * 3)()

        def call(cr, ch, rec, hits):
            rc = eng._lib.mrg_trf_classify(
                eng._h, d_words.data_ptr(), W, n + pad, d_lens.data_ptr(), None if d_nmask is None else d_nmask.data_ptr(), n,
                d_pass.data_ptr(), 2, 3, eng.libs["mature_trna"], eng.libs["pre_trna"], desc.ctypes.data, desc.shape[0],
                clusters.ctypes.data, clusters.shape[0], et.words.ctypes.data, et.plane.ctypes.data, et.words.shape[0], cr, ch,
                None if rec is None else rec.data_ptr(), None if hits is None else hits.data_ptr(), counts, None,
                eng._stream_ptr())
            assert rc == 0, eng._lib.mrg_last_error()
        call(0, 0, None, None)
        n2, n3 = int(counts[0]), int(counts[1])
        assert int(counts[2]) == 0
        cr = n2 + n3 if cap_rows is None else cap_rows
        rec = self.torch.full(((cr + GUARD) * 48,), PAT, dtype=self.torch.uint8, device=eng.device)
        if cap_hits is None:   # (count the kept alignments with a hit capacity of 0, as a caller would)
            call(cr, 0, rec, None)
            cap_hits = int(counts[2])
        hits = self.torch.full(((cap_hits + GUARD) * 16,), PAT, dtype=self.torch.uint8, device=eng.device)
        call(cr, cap_hits, rec, hits)
        assert (int(counts[0]), int(counts[1])) == (n2, n3)
        rows, kept = min(n2 + n3, cr), int(counts[2])
        raw_r, raw_h = rec.cpu().numpy(), hits.cpu().numpy()
        assert (raw_r[rows * 48:] == PAT).all(), "a record behind row %d (capacity %d)" % (rows, cr)
        assert (raw_h[min(kept, cap_hits) * 16:] == PAT).all(), "an alignment behind the capacity %d (%d kept)" % (cap_hits, kept)
        return (raw_r[:rows * 48].view(np.int32).reshape(rows, 12), raw_h[:min(kept, cap_hits) * 16].view(np.int32).reshape(-1, 4),
                n2, n3, kept)

    def model_rows(self, mature, trailer, index_of=None):
        return model.rows(self.et, self.tables, self.pre, mature, trailer, self.lister, index_of)

    def check(self, mature, trailer, W=None, order=None):
        """The reads through the device call (array order `order`: a permutation of mature + trailer, default as given)
        equal the model's rows."""
        reads = list(mature) + list(trailer)
        order = list(range(len(reads))) if order is None else list(order)
        arr = [reads[i] for i in order]
        words, lens, nmask = pack.pack_reads(arr, W)
        pass_id = np.array([2 if i < len(mature) else 3 for i in order], dtype=np.int8)
        rec, hits, n2, n3, kept = self.call(words, lens, nmask, pass_id, pad=3)
        at = {}
        for j, i in enumerate(order):
            at.setdefault(reads[i], j)
        m = [reads[i] for i in sorted(range(len(mature)), key=order.index)]
        t = [reads[i] for i in sorted(range(len(mature), len(reads)), key=order.index)]
        want_rec, want_hits = self.model_rows(m, t, at)
        assert (n2, n3, kept) == (len(m), len(t), want_hits.shape[0])
        same_rows(self.et, rec, hits, want_rec, want_hits, m + t)
        return rec, hits


def same_rows(et, rec, hits, want_rec, want_hits, reads=None):
    assert np.array_equal(hits, want_hits), first_diff(hits, want_hits, reads, rec)
    cols = [0, 1, 2, 3, 4, 6, 7, 8, 9, 10, 11]
    assert np.array_equal(rec[:, cols], want_rec[:, cols]), first_diff(rec, want_rec, reads)
    assert model.cluster_key(et, rec) == model.cluster_key(et, want_rec)


def first_diff(got, want, reads=None, rec=None):
    if got.shape != want.shape:
        return "shapes %s, model %s" % (got.shape, want.shape)
    r = int(np.nonzero((got != want).any(axis=1))[0][0])
    return "row %d%s: %s, model %s" % (r, "" if reads is None or rec is not None else " " + reads[r], got[r].tolist(), want[r].tolist())


# ---------------------------------------------------------------- the golden world
@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "trf.json")) as fh:
        return json.load(fh)


def test_golden_world_rows_equal_the_models(golden, native_lib, tmp_path):
    from tests.test_trf import write_world
    write_world(golden, str(tmp_path))
    tables = trf.load_trf_tables(str(tmp_path), "human")
    w = World({k: tuple(golden["libraries"][k]) for k in ("mature_trna", "pre_trna")}, tables)
    sd = golden["state"]["seqDic"]
    reads = list(sd)
    words, lens, nmask = pack.pack_reads(reads)
    pass_id = np.array([2 if sd[s]["annot"][3] != "" else 3 if sd[s]["annot"][4] != "" else -1 for s in reads], dtype=np.int8)
    rec, hits, n2, n3 = w.eng.trf_classify(w.et, words, lens, nmask, pass_id)
    mature = [s for s in reads if sd[s]["annot"][3] != ""]
    trailer = [s for s in reads if sd[s]["annot"][4] != ""]
    assert (n2, n3) == (173, 74)
    content = copy.deepcopy(golden["expected"]["trfContentDic_after_cascade"])
    want_rec, want_hits = model.rows(w.et, tables, w.pre, mature, trailer, None, {s: i for i, s in enumerate(reads)}, content)
    same_rows(w.et, rec, hits, want_rec, want_hits, mature + trailer)
    assert sum(int(r[9]) == 2 for r in rec) == 57 and set(rec[:, 7].tolist()) <= {0, 1, 2}


# ---------------------------------------------------------------- enumerated edges
def edge_world():
    rng = np.random.default_rng(77)
    X = rnd_seq(rng, 76)
    rep = rnd_seq(rng, 20)
    R = rep + rnd_seq(rng, 18) + rep + rnd_seq(rng, 18)                          # one 20-mer at offsets 0 and 38
    C19 = rnd_seq(rng, 76)
    U = rnd_seq(rng, 76)
    LONG = rnd_seq(rng, 300)
    PX = rnd_seq(rng, 76)                                                       # "pre" in its name, not "pre_"
    P1, P2 = rnd_seq(rng, 40), rnd_seq(rng, 40)
    mature = (["tRNA-x", "tRNA-rep", "tRNA-c19", "tRNA-und", "tRNA-long", "prex-tRNA"], [X, R, C19, U, LONG, PX])
    pre = (["pre_one_trailer", "pre_two_trailer", "prex-tRNA"], [P1, P2, PX[:20]])
    stru = {n: {"seq": s, "stru": STRU, "anticodonStart": 34, "anticodonEnd": 36} for n, s in zip(*mature)}
    aa = {n: {"aaType": "Gly", "anticodon": "GCC"} for n in mature[0] + pre[0]}
    aa["tRNA-und"] = {"aaType": "Und", "anticodon": "NNN"}
    und = U[:12] + "N" + U[13:30]
    clusters = {
        "tRNA-x": {trf.add_dash_new(X[:30], 76, 1, 30): "tRNA-x_Cluster1"},
        "tRNA-rep": {trf.add_dash_new(R[:20], 76, 1, 20): "tRNA-rep_Cluster1", trf.add_dash_new(R[38:58], 76, 39, 58): "tRNA-rep_Cluster2"},
        "tRNA-c19": {trf.add_dash_new(C19[:19], 19, 1, 19): "tRNA-c19_Cluster1"},
        "tRNA-und": {trf.add_dash_new(und, 76, 1, 30): "tRNA-und_Cluster1"},
        "tRNA-long": {trf.add_dash_new(LONG[:40], 300, 1, 40): "tRNA-long_Cluster1",
                      trf.add_dash_new(LONG[59:130], 300, 60, 130): "tRNA-long_Cluster2",
                      trf.add_dash_new(LONG[200:], 300, 201, 300): "tRNA-long_Cluster3"},
        "prex-tRNA": {trf.add_dash_new(PX[:18], 20, 1, 18): "prex-tRNA_Cluster1"},
        "pre_one_trailer": {trf.add_dash_new(P1[:20], 40, 1, 20): "pre_one_trailer_Cluster1"},
    }
    names = sorted({c for d in clusters.values() for c in d.values()})
    tables = {"trnaStruDic": stru, "trnaAAanticodonDic": aa, "duptRNA2UniqueDic": {}, "tRNAtrfDic": clusters,
              "trfMergedNameDic": {c: c + "_m" for c in names}, "trfMergedList": [c + "_m" for c in names]}
    seqs = dict(X=X, R=R, rep=rep, C19=C19, U=U, LONG=LONG, PX=PX, P1=P1, P2=P2)
    return {"mature_trna": mature, "pre_trna": pre}, tables, seqs


@pytest.fixture(scope="module")
def edges(native_lib):
    libs, tables, seqs = edge_world()
    return World(libs, tables), seqs


def test_every_type_at_both_sides_of_its_boundaries(edges):
    w, s = edges
    X, n, anticodon = s["X"], 76, 33
    reads = [X]                                                      # start 0 with the whole length
    reads += [X[:last + 1] for last in range(anticodon - 3, anticodon + 3)]          # 5'-half: anticodon - 2 .. + 1
    for start in range(anticodon - 2, anticodon + 4):                # 3'-half: start anticodon - 1 .. + 2
        reads += [X[start:last + 1] for last in range(n - 4, n)]     # last n - 3 .. n - 1, and one in front
    reads += [X[1:30], X[5:n - 4], X[1:n], X[:n - 1]]
    rec, hits = w.check(sorted(set(reads), key=reads.index), [])
    assert set(hits[:, 3].tolist()) == {1, 2, 3, 4, 5, 6}
    by_read = {r: trf.TRF_TYPES[t] for r, t in zip(sorted(set(reads), key=reads.index), rec[:, 4].tolist())}
    assert by_read[X] == "tRF-whole" and by_read[X[:anticodon - 2]] == "5'-tRF" and by_read[X[:anticodon - 1]] == "5'-half"
    assert by_read[X[:anticodon + 2]] == "5'-half" and by_read[X[:anticodon + 3]] == "5'-tRF"
    assert by_read[X[anticodon - 2:n]] == "3'-tRF" and by_read[X[anticodon - 1:n]] == "3'-half"
    assert by_read[X[anticodon + 2:n - 2]] == "3'-half" and by_read[X[anticodon + 3:n]] == "3'-tRF"
    assert by_read[X[5:n - 4]] == "i-tRF" and by_read[X[1:30]] == "i-tRF"


def test_offsets_distances_overhang_and_n(edges):
    w, s = edges
    X, C19, U, PX = s["X"], s["C19"], s["U"], s["PX"]
    flip = {"A": "C", "C": "G", "G": "T", "T": "A"}
    mature = [s["rep"],                                  # one tRNA at two offsets: the lowest is kept
              X[4:34], X[4:35],                          # distance exactly 8 and 9
              X[:29] + flip[X[29]], X[2:17] + flip[X[17]] + X[18:32],   # a -v 1 substitution counts once
              C19[:21], C19[:25], C19[3:19], C19[10:40],  # overhanging a 19-base predefined string
              U[:12] + "N" + U[13:30], U[:30], U[:5] + "N" + U[6:30], U[2:12] + "N" + U[13:33],   # N on both, on one side
              PX[:18], PX[10:40], PX[30:60]]             # the pad of add_dash_new goes negative (template of 20)
    rec, hits = w.check(mature, [])
    assert rec[0, 9] == 1 and rec[0, 2] == 0 and hits[0].tolist()[:3] == [1, 0, 19]
    assert rec[1, [6, 7]].tolist() == [8, trf.KIND_ASSIGNED] and rec[2, [6, 7]].tolist() == [9, trf.KIND_UNDEF]
    assert rec[3, 6] == 1 and rec[5, [6, 7]].tolist() == [4, trf.KIND_ASSIGNED] and rec[6, 6] == 12
    assert rec[9, 6] == 0 and rec[10, 6] == 1 and rec[11, 6] == 2
    assert rec[15, 3] >= 20 and rec[15, 7] == trf.KIND_UNDEF


def test_trailer_tails_and_group_order(edges):
    w, s = edges
    P1, P2 = s["P1"].rstrip("T"), s["P2"].rstrip("T")
    a, b = P1[:18].rstrip("T"), P2[5:25].rstrip("T")
    one = [a + "T" * t for t in (3, 4, 10)]
    two = [b + "T" * t for t in (10, 3, 4)]
    bad = [a + "TT", a[:10] + "TTTT", a[:11] + "TTT"]          # 2 T's; 10 nt left; 11 nt left (listed)
    trailer = [one[0], two[0], one[1], bad[0], two[1], one[2], bad[1], two[2], bad[2]]
    mature = [s["X"][:30]]
    rec, hits = w.check(mature, trailer, order=[1, 2, 0, 3, 4, 5, 6, 7, 8, 9])
    kinds = rec[1:, 7].tolist()
    assert kinds[3] == trf.KIND_RANGE and kinds[6] == trf.KIND_RANGE and kinds[8] != trf.KIND_RANGE
    assert rec[1:, 10].tolist() == [3, 10, 4, 2, 3, 10, 4, 4, 3]
    assert (rec[[1, 2, 3], 4] == 0).all() and (rec[1, 3] == len(a) - 1)
    # the order of the tsv: the mature row, then the groups by first appearance, array order inside
    words, lens, nmask = pack.pack_reads([trailer[0], trailer[1], mature[0]] + trailer[2:])
    order = trf.row_order(rec, 1, words, lens, nmask)
    got = [int(rec[i, 0]) for i in order]
    assert got == [2, 0, 3, 4, 6, 1, 5, 8, 7, 9]   # (a rejected read is grouped by what is left of it: the route raises anyway)


@pytest.mark.parametrize("W", [1, 2, 4, 8])
def test_read_lengths_under_every_word_count(edges, W):
    w, s = edges
    LONG = s["LONG"]
    flip = {"A": "C", "C": "G", "G": "T", "T": "A"}
    reads = []
    for L in (16, 32, 33, 64, 65, 255):
        if L > 32 * W:
            continue
        for start in (0, 3, 31, 45, 59, 300 - L):
            if start + L > 300:
                continue
            r = LONG[start:start + L]
            reads += [r, r[:L - 1] + flip[r[L - 1]], r[:L // 2] + "N" + r[L // 2 + 1:]]
    reads = sorted(set(reads), key=reads.index)
    rec, hits = w.check(reads, [], W=W)
    assert (rec[:, 7] <= trf.KIND_UNDEF).all() and (rec[:, 9] == 1).all()


def test_random_reads_against_the_model(edges):
    w, s = edges
    rng = np.random.default_rng(5)
    mature, trailer = [], []
    pools = [s[k] for k in ("X", "R", "C19", "U", "LONG", "PX")]
    while len(mature) < 2400:
        seq = pools[int(rng.integers(len(pools)))]
        L = int(rng.integers(14, min(len(seq), 120) + 1))
        at = int(rng.integers(0, len(seq) - L + 1))
        r = list(seq[at:at + L])
        roll = rng.random()
        if roll < 0.3:
            r[int(rng.integers(L))] = "ACGT"[int(rng.integers(4))]
        elif roll < 0.4:
            r[int(rng.integers(L))] = "N"
        mature.append("".join(r))
    while len(trailer) < 600:
        seq = (s["P1"], s["P2"])[int(rng.integers(2))]
        L = int(rng.integers(9, 31))
        at = int(rng.integers(0, len(seq) - L + 1))
        trailer.append(seq[at:at + L] + "T" * int(rng.integers(1, 12)))
    mature += [rnd_seq(rng, 22) for _ in range(40)]                  # (reads that align nowhere: no candidate)
    mature = sorted(set(mature), key=mature.index)
    trailer = sorted(set(trailer) - set(mature), key=trailer.index)
    order = rng.permutation(len(mature) + len(trailer)).tolist()
    rec, hits = w.check(mature, trailer, order=order)
    kinds = set(rec[:, 7].tolist())
    assert {trf.KIND_ASSIGNED, trf.KIND_UNDEF, trf.KIND_RANGE, trf.KIND_NONE} <= kinds and rec.shape[0] > 2500


# ---------------------------------------------------------------- selection, capacity, guards
@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097, 70001])
def test_selection_order_capacity_and_guards(edges, n):
    w, s = edges
    X, P1 = s["X"], s["P1"].rstrip("T")
    distinct = [X[:30], X[40:76], s["rep"], s["C19"][:21], s["U"][:30], P1[:18].rstrip("T") + "TTT", P1[3:20].rstrip("T") + "TTTT",
                X[10:20] + "ACGTACGT"]
    is_trailer = [False] * 5 + [True, True, False]
    rng = np.random.default_rng(n)
    pick = rng.integers(0, len(distinct), n)
    claimed = rng.random(n) < 0.7
    pass_id = np.where(claimed, np.where(np.array(is_trailer)[pick], 3, 2), rng.integers(4, 9, n)).astype(np.int8)
    words8, lens8, nmask8 = pack.pack_reads(distinct, 2)
    words, lens = np.ascontiguousarray(words8[:, pick]), lens8[pick]
    assert nmask8 is None
    # the model, once per distinct read
    m_rec, m_hits = w.model_rows([d for d, t in zip(distinct, is_trailer) if not t], [d for d, t in zip(distinct, is_trailer) if t])
    slot = {d: r for r, d in enumerate([d for d, t in zip(distinct, is_trailer) if not t] + [d for d, t in zip(distinct, is_trailer) if t])}
    idx = np.concatenate([np.nonzero(pass_id == 2)[0], np.nonzero(pass_id == 3)[0]])
    src = np.array([slot[distinct[int(pick[i])]] for i in idx], dtype=np.int64)
    want_rec = m_rec[src].copy() if idx.size else m_rec[:0].copy()
    want_rec[:, 0] = idx
    counts = want_rec[:, 9].astype(np.int64)
    want_rec[:, 8] = np.where(counts > 0, np.cumsum(counts) - counts, 0)
    pieces = [m_hits[int(a):int(a) + int(c)] for a, c in zip(m_rec[src, 8], m_rec[src, 9])] if idx.size else []
    want_hits = np.concatenate(pieces) if pieces else m_hits[:0]
    k, h = idx.size, want_hits.shape[0]
    for cap_rows, cap_hits in ((None, None), (k // 2, None), (k, h // 3), (k + 5, h + 5), (0, 0)):
        rec, hits, n2, n3, kept = w.call(words, lens, None, pass_id, cap_rows, cap_hits, pad=2)
        assert (n2, n3) == (int((pass_id == 2).sum()), int((pass_id == 3).sum()))
        rows = k if cap_rows is None else min(k, cap_rows)
        assert rec.shape[0] == rows and np.array_equal(rec[:, 0], idx[:rows])
        rows_hits = int(want_rec[:rows, 9].sum())
        assert kept == rows_hits
        same_rows(w.et, rec, hits, want_rec[:rows], want_hits[:min(rows_hits, hits.shape[0])])
        assert hits.shape[0] == (rows_hits if cap_hits is None else min(rows_hits, cap_hits))


def test_a_read_with_more_than_64_kept_alignments(native_lib):
    rng = np.random.default_rng(9)
    common = rnd_seq(rng, 24)
    names = ["tRNA-m%02d" % i for i in range(70)]
    seqs = [rnd_seq(rng, int(rng.integers(5, 40))) + common + rnd_seq(rng, 20) + (common if i % 7 == 0 else "") for i in range(70)]
    stru = {n: {"seq": q, "stru": STRU, "anticodonStart": 34, "anticodonEnd": 36} for n, q in zip(names, seqs)}
    aa = {n: {"aaType": "Ala", "anticodon": "AGC"} for n in names + ["pre_p_trailer"]}
    dup = {names[i]: names[i - 1] for i in range(1, 70, 2)}
    clusters = {names[0]: {trf.add_dash_new(seqs[0][:30], len(seqs[0]), 1, 30): names[0] + "_Cluster1"}}
    tables = {"trnaStruDic": stru, "trnaAAanticodonDic": aa, "duptRNA2UniqueDic": dup, "tRNAtrfDic": clusters,
              "trfMergedNameDic": {names[0] + "_Cluster1": "m"}, "trfMergedList": ["m"]}
    w = World({"mature_trna": (names, seqs), "pre_trna": (["pre_p_trailer"], [rnd_seq(rng, 40)])}, tables)
    rec, hits = w.check([common, seqs[3][:30], common[:20]], [])
    assert rec[0, 9] == 70 and rec[0, 1] == 0 and hits.shape[0] >= 141


# ---------------------------------------------------------------- unresolvable entries
def test_an_unresolvable_entry_raises_only_when_a_read_reaches_it(native_lib, tmp_path):
    from mirge_amd import columnar
    from tests.test_trf_native import T2, PRE1, hand_world
    libs, tables, pre = hand_world()
    w = World(libs, tables, pre)
    seqs = dict(zip(*libs["mature_trna"]))
    log = {"quantStats": [{"maturetrnaReads": 5, "pretrnaReads": 1}]}

    def both(mature, trailer):
        reads = mature + trailer
        sd = model.seq_dic(mature, trailer, [[1]] * len(reads))
        words, lens, nmask = pack.pack_reads(reads)
        pass_id = np.array([2] * len(mature) + [3] * len(trailer), dtype=np.int8)
        rec, hits, n2, n3 = w.eng.trf_classify(w.et, words, lens, nmask, pass_id)

        def python():
            content = {}
            trf.collect_trf_content(content, sd, ["s"], tables["trnaStruDic"], pre, w.lister)
            trf.write_trf_tables(str(tmp_path), ["s"], copy.deepcopy(log), content, tables, pre)

        def arrays():
            columnar.write_trf_tables(str(tmp_path), ["s"], log, words, lens, nmask, np.ones((len(reads), 1), np.uint32), rec,
                                      hits, n2, w.et)
        return python, arrays, rec, hits
    good = [T2[:30], T2[20:50]]
    python, arrays, rec, hits = both(good, [PRE1[:12] + "TTT"])
    python()
    ref = {fn: open(os.path.join(str(tmp_path), fn), "rb").read() for fn in ("tRFs.potential.report.tsv", "tRF.Counts.csv")}
    arrays()
    assert ref == {fn: open(os.path.join(str(tmp_path), fn), "rb").read() for fn in ref}
    for read, kind in ((seqs["tRNA-noaa"][:25], None), (seqs["tRNA-dupgone"][-30:], trf.KIND_UNRESOLVABLE),
                       (T2[50:76], trf.KIND_ASSIGNED), (seqs["tRNA-nostru"][3:30], trf.KIND_UNRESOLVABLE)):
        python, arrays, rec, hits = both(good + [read], [])
        if kind is not None:
            assert rec[2, 7] == kind
        with pytest.raises(KeyError) as want:
            python()
        with pytest.raises(KeyError) as got:
            arrays()
        assert repr(got.value) == repr(want.value), read
    assert hits[-1, 3] == trf.TYPE_UNRESOLVABLE


# ---------------------------------------------------------------- the command line
def golden_fastqs(golden, tmp_path, extra=()):
    fastqs = []
    for si, (name, reads) in enumerate(zip(golden["sample_list"], golden["samples"])):
        p = str(tmp_path / name)
        with open(p, "w") as fh:
            for k, r in enumerate(list(reads) + list(extra) * (si + 1)):
                fh.write("@r%d\n%s\n+\n%s\n" % (k, r, "I" * len(r)))
        fastqs.append(p)
    return fastqs


def run_trf(tmp_path, root, fastqs, label, extra=()):
    from mirge_amd import cli
    out = tmp_path / label
    out.mkdir()
    res = cli.annotate_main(cli.build_parser().parse_args(
        ["annotate", "-s"] + fastqs + ["-lib", root, "-sp", "human", "-o", str(out), "-trf"] + list(extra)))
    files = {}
    for base, _, fns in os.walk(res["outdir"]):
        for fn in fns:
            path = os.path.join(base, fn)
            if fn.startswith(("tRF", "discarded")) or "tRFs.samples.tmp" in path:
                files[os.path.relpath(path, res["outdir"])] = open(path, "rb").read()
    return res["outdir"], files


def test_cli_trf_with_and_without_trf_host(golden, native_lib, tmp_path, monkeypatch):
    from mirge_amd import columnar
    from tests.test_trf import check_files, write_world
    root = str(tmp_path / "libs")
    write_world(golden, root)
    fastqs = golden_fastqs(golden, tmp_path)
    calls = []
    real = columnar.write_trf_tables
    monkeypatch.setattr(columnar, "write_trf_tables", lambda *a, **k: calls.append(1) or real(*a, **k))
    new_dir, new = run_trf(tmp_path, root, fastqs, "new")
    assert calls == [1]
    old_dir, old = run_trf(tmp_path, root, fastqs, "old", ["--trf-host"])
    assert calls == [1]
    assert new == old and len(new) > 4 and any("tRFs.samples.tmp" in fn for fn in new)
    check_files(golden, new_dir)


def test_a_trna_read_beyond_255_nt_takes_the_record_route(golden, native_lib, tmp_path, monkeypatch):
    """A read of 263 nt claimed by the mature-tRNA pass is not in the packed arrays: the run does not call the array route."""
    from mirge_amd import columnar
    from tests.test_trf import write_world
    rng = np.random.default_rng(3)
    body = rnd_seq(rng, 300)
    g = copy.deepcopy(golden)
    name = "Homo_sapiens_tRNA-Xxx-AAA-99-1"
    g["libraries"]["mature_trna"][0].append(name)
    g["libraries"]["mature_trna"][1].append(body)
    g["tables"]["_trna.str"] = g["tables"]["_trna.str"].rstrip("\n") + "\n>%s\n%s\n%s\n" % (name, body, "." * 33 + "XXX" + "." * 264)
    g["tables"]["_trna_aminoacid_anticodon.csv"] = g["tables"]["_trna_aminoacid_anticodon.csv"].rstrip("\n") + "\n%s,Xxx,AAA\n" % name
    root = str(tmp_path / "libs")
    write_world(g, root)
    long_read = body[5:268]
    fastqs = golden_fastqs(g, tmp_path, [long_read])
    calls = []
    real = columnar.write_trf_tables
    monkeypatch.setattr(columnar, "write_trf_tables", lambda *a, **k: calls.append(1) or real(*a, **k))
    # the record route is what such a run took before the array route existed, and it ends as it ended then:
    # trf.engine_lister packs the reads for the listing, and pack_reads does not describe a read beyond 255 nt
    for label, extra in (("new", []), ("old", ["--trf-host"])):
        with pytest.raises(ValueError, match="longer than 255 nt"):
            run_trf(tmp_path, root, fastqs, label, extra)
    assert calls == []
    # without that read the same world takes the array route
    new_dir, new = run_trf(tmp_path, root, golden_fastqs(g, tmp_path), "short")
    assert calls == [1]
