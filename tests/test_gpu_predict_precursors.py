"""Predict mode's precursor candidates on the GPU (-m gpu): mrg_predict_precursors and mrg_predict_precursor_bases on
hand-made arrays against the model (tests/predict_precursors_model.py) with guard words behind every output -- group counts
around the block size, windows at every residue of the 16 bases of a text word on both strands, segment boundaries and N
gaps, two genome parts of two entries, the clamps, unwritten groups, contradicting arrays --, the golden worlds of the
reference byte for byte, and predict.map_and_cluster(..., precursors=True), `predict clusters --precursors` and
`annotate --novel-precursors` end to end against the model run over the feature file the same run wrote."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import predict_features_cases as feature_cases
from tests import predict_features_model as features_model
from tests import predict_precursors_cases as cases
from tests import predict_precursors_model as model

pytestmark = pytest.mark.gpu

GOLD = cases.golden()
WORLDS = GOLD["worlds"]
GUARD = 64
SUFFIX = "_vs_representative_seq_modified_selected_sorted.tsv"
SIGNED = {np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}
HEADER = features_model.HEADER_HEAD + features_model.HEADER_TAIL
COLUMNS = HEADER.rstrip("\n").split("\t")
FEATURE_KEYS = {"row_group", "row_status", "row_diag", "row_ident", "group_off", "group_cluster", "group_sum", "group_pass", "group_host",
                "valid", "frame", "exact", "nine", "nb_t", "nb_up", "nb_down", "nb_flags", "order", "n_groups", "n_passed", "n_sorted",
                "host_results"}


@pytest.fixture(scope="module")
def engine(native_lib):
    from mirge_amd.engine import Engine
    eng = Engine(0)
    yield eng
    eng.close()


def rand_seq(rng, L):
    return "".join("ACGT"[c] for c in rng.integers(0, 4, L))


@pytest.fixture(scope="module")
def genome(engine):
    """Two parts of two entries: one segment; three segments (gaps of 30 and of 1); N runs at both ends; the last entry."""
    from mirge_amd.index import FmIndex
    rng = np.random.default_rng(2024)
    a2 = list(rand_seq(rng, 400))
    a2[100:130] = "N" * 30
    a2[250:251] = "N"
    b1 = list(rand_seq(rng, 300))
    b1[0:20] = "N" * 20
    b1[280:300] = "N" * 20
    chroms = {"chrA1": rand_seq(rng, 300), "chrA2": "".join(a2), "chrB1": "".join(b1), "chrB2": rand_seq(rng, 257)}
    names = list(chroms)
    parts = [FmIndex.build(names[:2], [chroms[n] for n in names[:2]]), FmIndex.build(names[2:], [chroms[n] for n in names[2:]])]
    keys = ["precursor_test:A", "precursor_test:B"]
    for k, ix in zip(keys, parts):
        engine.add_library(k, ix, exact_dict=False)
    return dict(chroms=chroms, names=names, parts=parts, keys=keys, entry_len=np.array([len(chroms[n]) for n in names], np.uint32))


class Dev:
    """Device buffers with guard words behind the outputs."""

    def __init__(self, engine):
        import torch
        self.torch, self.engine, self.outs = torch, engine, []

    def up(self, a, dtype):
        a = np.array(a, dtype=dtype)          # (a copy: torch wants writable memory)
        if a.size == 0:
            a = np.zeros(1, dtype)
        return self.torch.from_numpy(a.reshape(-1).view(SIGNED.get(a.dtype, a.dtype))).to(self.engine.device)

    def out(self, n, dtype):
        dtype = np.dtype(dtype)
        a = np.full(int(n) + GUARD, 0x5A, dtype=SIGNED.get(dtype, dtype))
        t = self.torch.from_numpy(a).to(self.engine.device)
        self.outs.append((t, int(n)))
        return t

    def tmp(self, n_order):
        need = C.c_uint64()
        assert self.engine._lib.mrg_predict_precursor_temp_bytes(int(n_order), C.byref(need)) == 0
        return self.torch.empty(max(int(need.value), 64), dtype=self.torch.uint8, device=self.engine.device)

    def guards_intact(self, untouched=False):
        for t, n in self.outs:
            tail = t.cpu().numpy()[0 if untouched else n:]
            assert tail.shape[0] == GUARD + (n if untouched else 0) and (tail == 0x5A).all()
        return True


def host(t, n, dtype):
    return t.cpu().numpy()[:n].view(dtype)


def call_windows(engine, order, group_cluster, frame, valid, cl, entry_len, expect_error=False):
    d = Dev(engine)
    S, G, K, E = len(order), len(group_cluster), len(cl["entry"]), len(entry_len)
    ins = [d.up(order, np.uint32), d.up(group_cluster, np.uint32), d.up(frame, np.int32), d.up(valid, np.uint8), d.up(cl["entry"], np.uint32),
           d.up(cl["strand"], np.uint8), d.up(cl["start"], np.uint32), d.up(cl["end"], np.uint32), d.up(entry_len, np.uint32)]
    written, rg, lo, hi = d.out(S, np.uint8), d.out(2 * S, np.uint32), d.out(2 * S, np.uint32), d.out(2 * S, np.uint32)
    off = d.out(2 * S + 1, np.uint64)
    tmp = d.tmp(S)
    W, total = C.c_uint64(99), C.c_uint64(99)
    p = lambda t: t.data_ptr()
    rc = engine._lib.mrg_predict_precursors(engine._h, S, p(ins[0]), G, p(ins[1]), p(ins[2]), p(ins[3]), K, p(ins[4]), p(ins[5]), p(ins[6]),
                                            p(ins[7]), E, p(ins[8]), p(written), p(rg), p(lo), p(hi), p(off), C.byref(W), C.byref(total),
                                            p(tmp), tmp.numel(), engine._stream_ptr())
    assert d.guards_intact()
    if expect_error:
        assert rc == -1 and W.value == 0 and total.value == 0
        return None
    assert rc == 0, engine._lib.mrg_last_error()
    W = int(W.value)
    return dict(written=host(written, S, np.uint8), rec_group=host(rg, 2 * W, np.uint32), rec_lo=host(lo, 2 * W, np.uint32),
                rec_hi=host(hi, 2 * W, np.uint32), rec_off=host(off, 2 * W + 1, np.uint64), n_written=W, seq_len=int(total.value))


def call_bases(engine, genome, rec_group, rec_lo, rec_hi, rec_off, group_cluster, cl_entry, cl_strand, expect_error=False, entry_len=None,
               entry_base=None):
    d = Dev(engine)
    n, total = len(rec_group), int(rec_off[-1])
    entry_len = genome["entry_len"] if entry_len is None else entry_len
    ins = [d.up(rec_group, np.uint32), d.up(rec_lo, np.uint32), d.up(rec_hi, np.uint32), d.up(rec_off, np.uint64),
           d.up(group_cluster, np.uint32), d.up(cl_entry, np.uint32), d.up(cl_strand, np.uint8), d.up(entry_len, np.uint32)]
    seq = d.out(total, np.uint8)
    tmp = d.tmp(0)
    lids = np.array([engine.libs[k] for k in genome["keys"]], dtype=np.int32)
    ebase = np.array([0, 2] if entry_base is None else entry_base, dtype=np.uint32)
    p = lambda t: t.data_ptr()
    rc = engine._lib.mrg_predict_precursor_bases(engine._h, n, p(ins[0]), p(ins[1]), p(ins[2]), p(ins[3]), len(group_cluster), p(ins[4]),
                                                 len(cl_entry), p(ins[5]), p(ins[6]), len(entry_len), p(ins[7]), len(lids), lids.ctypes.data,
                                                 ebase.ctypes.data, p(seq), total, p(tmp), tmp.numel(), engine._stream_ptr())
    if expect_error:
        assert rc == -1
        assert d.guards_intact(untouched=True)          # nothing written, in front of the guards or behind them
        return None
    assert rc == 0, engine._lib.mrg_last_error()
    assert d.guards_intact()
    return host(seq, total, np.uint8).tobytes()


def feature_line(ch, start, end, strand, H, T, hu, tu, number):
    f = ["."] * len(COLUMNS)
    f[5] = "smp:miRCluster_%d_%d:%s:%d_%d%s" % (number, end - start + 1, ch, start, end, strand)
    f[COLUMNS.index("alignedClusterSeq")] = "-" * H + "A" * (end - start + 1) + "-" * T
    f[COLUMNS.index("headUnstableLength")], f[COLUMNS.index("tailUnstableLength")] = str(hu), str(tu)
    return "\t".join(f) + "\n"


def random_groups(rng, genome, n):
    """n groups on the genome: (entry name, start, end, strand, H, T, head, tail_add, written); about one in eight has a
    stable stretch of six columns and no line."""
    out = []
    for g in range(n):
        ch = genome["names"][int(rng.integers(0, 4))]
        L = len(genome["chroms"][ch])
        length = int(rng.integers(16, 26))
        start = int(rng.integers(1, L - length + 2))
        H, T, head, tail_add = (int(rng.integers(0, k)) for k in (4, 4, 5, 8))
        if rng.integers(0, 8) == 0:      # (H + length + T) + pads - head - tail_add = 6
            H, T, head, tail_add = 0, 0, 5, 6
            length = 17
            start = min(start, L - length + 1)
        out.append((ch, start, start + length - 1, "+-"[int(rng.integers(0, 2))], H, T, head, tail_add))
    return out


def stable_length(H, L, T, head, tail_add):
    return H + L + T + max(0, 3 - head) + max(0, 6 - tail_add) - head - tail_add


def run_groups(engine, genome, groups, order):
    """The groups through both device calls and the writer against the model over the lines of the written ones."""
    from mirge_amd import predict
    from mirge_amd.index import FmIndex
    G = len(groups)
    cl = dict(entry=np.array([genome["names"].index(g[0]) for g in groups], np.uint32), strand=np.array([g[3] == "-" for g in groups], np.uint8),
              start=np.array([g[1] for g in groups], np.uint32), end=np.array([g[2] for g in groups], np.uint32))
    frame = np.array([(g[4], g[5], g[6], -g[7] - 1) for g in groups], np.int32).reshape(G, 4)
    group_cluster = np.arange(G, dtype=np.uint32)[::-1].copy()     # group g is cluster G - 1 - g
    cl = {k: v[::-1].copy() for k, v in cl.items()}
    lines_of = [j for j in order if stable_length(groups[j][4], groups[j][2] - groups[j][1] + 1, groups[j][5], groups[j][6], groups[j][7]) >= 7]
    text = HEADER + "".join(feature_line(*groups[j], number=j + 1) for j in lines_of)
    want = model.records(text, genome["chroms"])
    got = call_windows(engine, order, group_cluster, frame, np.ones(G, np.uint8), cl, genome["entry_len"])
    has_line = set(lines_of)
    assert got["n_written"] == len(lines_of) and list(np.flatnonzero(got["written"])) == [k for k, j in enumerate(order) if j in has_line]
    assert list(got["rec_group"]) == [j for j in lines_of for _ in range(2)]
    assert list(got["rec_lo"]) == [r[3] for r in want] and list(got["rec_hi"]) == [r[4] for r in want]
    assert list(got["rec_off"]) == list(np.cumsum([0] + [len(r[5]) for r in want])) and got["seq_len"] == sum(len(r[5]) for r in want)
    seq = call_bases(engine, genome, got["rec_group"], got["rec_lo"], got["rec_hi"], got["rec_off"], group_cluster, cl["entry"], cl["strand"])
    assert seq == "".join(r[5] for r in want).encode()
    return text, dict(got, seq=seq), group_cluster, cl


@pytest.mark.parametrize("n", [0, 1, 2, 255, 256, 257, 4097])
def test_group_counts_against_the_model(engine, genome, tmp_path, n):
    from mirge_amd import predict
    from mirge_amd.index import FmIndex
    rng = np.random.default_rng(100 + n)
    groups = random_groups(rng, genome, n)
    order = [int(j) for j in rng.permutation(n)]
    text, got, group_cluster, cl = run_groups(engine, genome, groups, order)
    if n in (2, 257):       # the file from the device's arrays
        names = ["smp:miRCluster_%d_%d:%s:%d_%d%s" % (j + 1, g[2] - g[1] + 1, g[0], g[1], g[2], g[3]) for j, g in enumerate(groups)][::-1]
        lib = FmIndex.build(names, ["ACGT" * 5] * n)
        path = str(tmp_path / "p.fa")
        predict.write_precursors(path, genome["parts"], lib, cl["entry"], group_cluster, got)
        assert open(path).read() == model.run(text, genome["chroms"])
    if n == 4097:
        assert 0 < got["n_written"] < n


def test_unwritten_groups_are_dropped_from_the_records(engine, genome):
    groups = [("chrA1", 100, 117, "+", 0, 0, 4, 7), ("chrA1", 100, 117, "+", 0, 0, 5, 7), ("chrB2", 100, 117, "-", 0, 0, 5, 7),
              ("chrB2", 100, 117, "-", 0, 0, 4, 7)]
    assert [stable_length(g[4], 18, g[5], g[6], g[7]) for g in groups] == [7, 6, 6, 7]
    _, got, _, _ = run_groups(engine, genome, groups, [0, 1, 2, 3])
    assert list(got["written"]) == [1, 0, 0, 1] and list(got["rec_group"]) == [0, 0, 3, 3]


def test_clamps_overhangs_and_the_end_of_the_last_entry(engine, genome):
    last = len(genome["chroms"]["chrB2"])
    groups = [("chrA1", 40, 60, "+", 0, 0, 0, 0),            # precusor_1 clamped at 0
              ("chrA1", 15, 36, "-", 0, 0, 0, 0),            # both clamped at 0
              ("chrA1", 3, 20, "+", 2, 3, 1, 2),
              ("chrB2", last - 20, last, "+", 0, 0, 0, 0),    # a cluster ending at entry_len on the last entry: both clipped
              ("chrB2", last - 20, last, "-", 1, 2, 2, 1),
              ("chrB2", last - 60, last - 40, "+", 0, 0, 0, 0),  # e + 20 inside, e + 70 beyond
              ("chrA2", 140, 160, "-", 3, 0, 0, 3), ("chrB1", 30, 50, "+", 0, 3, 3, 0)]
    run_groups(engine, genome, groups, list(range(len(groups))))


def records_on(genome, windows):
    """Hand-made records [(entry name, strand, lo, hi)], each of its own cluster and group."""
    n = len(windows)
    entry = np.array([genome["names"].index(w[0]) for w in windows], np.uint32)
    strand = np.array([w[1] == "-" for w in windows], np.uint8)
    lo, hi = np.array([w[2] for w in windows], np.uint32), np.array([w[3] for w in windows], np.uint32)
    off = np.cumsum([0] + [w[3] - w[2] for w in windows]).astype(np.uint64)
    want = "".join(model.rna(genome["chroms"][w[0]][w[2]:w[3]], w[1]) for w in windows).encode()
    return dict(rec_group=np.arange(n, dtype=np.uint32), rec_lo=lo, rec_hi=hi, rec_off=off, group_cluster=np.arange(n, dtype=np.uint32),
                cl_entry=entry, cl_strand=strand), want


def test_windows_at_every_residue_of_a_text_word(engine, genome):
    windows = [(ch, s, lo, lo + n) for ch in ("chrA1", "chrB2") for s in "+-" for lo in range(40, 56) for n in range(1, 34)]
    r, want = records_on(genome, windows)
    assert {(w[2] % 16, w[3] % 16) for w in windows} == {(a, b) for a in range(16) for b in range(16)}
    assert call_bases(engine, genome, **r) == want


def test_segment_boundaries_and_n_gaps(engine, genome):
    spans = {"chrA2": [(90, 140), (110, 150), (80, 120), (105, 125), (99, 101), (129, 131), (240, 260), (250, 251), (0, 400), (130, 250),
                       (200, 200)],
             "chrB1": [(0, 30), (0, 20), (19, 21), (270, 300), (280, 300), (279, 281), (0, 300), (5, 15)],
             "chrA1": [(0, 300), (0, 1), (299, 300)], "chrB2": [(200, 257), (0, 257), (256, 257), (257, 257)]}
    windows = [(ch, s, lo, hi) for ch, v in spans.items() for lo, hi in v for s in "+-"]
    r, want = records_on(genome, windows)
    got = call_bases(engine, genome, **r)
    assert got == want
    assert b"N" * 30 in got and got.count(b"N") > 200 and set(got) <= set(b"ACGUN")


def test_contradicting_windows_inputs_are_errors(engine, genome):
    groups = random_groups(np.random.default_rng(5), genome, 40)
    G = len(groups)
    cl = dict(entry=np.array([genome["names"].index(g[0]) for g in groups], np.uint32), strand=np.array([g[3] == "-" for g in groups], np.uint8),
              start=np.array([g[1] for g in groups], np.uint32), end=np.array([g[2] for g in groups], np.uint32))
    frame = np.array([(g[4], g[5], g[6], -g[7] - 1) for g in groups], np.int32)
    gc, ok, order, elen = np.arange(G, dtype=np.uint32), np.ones(G, np.uint8), np.arange(G, dtype=np.uint32), genome["entry_len"]
    assert call_windows(engine, order, gc, frame, ok, cl, elen) is not None
    invalid = ok.copy()
    invalid[17] = 0
    call_windows(engine, order, gc, frame, invalid, cl, elen, expect_error=True)              # order names an invalid group
    assert call_windows(engine, np.delete(order, 17), gc, frame, invalid, cl, elen) is not None  # (not listed: fine)
    beyond = order.copy()
    beyond[3] = G
    call_windows(engine, beyond[:G - 1], gc, frame, ok, cl, elen, expect_error=True)          # a group >= G
    bad = gc.copy()
    bad[9] = G
    call_windows(engine, order, bad, frame, ok, cl, elen, expect_error=True)                  # a cluster >= K
    call_windows(engine, order, gc, frame, ok, dict(cl, entry=cl["entry"] + 4), elen, expect_error=True)   # an entry >= E
    # a window ending before the chromosome: H 60, L 5, tailAdd 30 is written (38 stable columns), e = 5 - 30
    one = dict(entry=[0], strand=[0], start=[1], end=[5])
    call_windows(engine, [0], [0], np.array([[60, 0, 0, -31]], np.int32), [1], one, elen, expect_error=True)
    with pytest.raises(ValueError, match="first base"):
        model.records(HEADER + feature_line("chrA1", 1, 5, "+", 60, 0, 0, 30, 1), genome["chroms"])
    assert engine._lib.mrg_predict_precursors(engine._h, 2, None, 1, None, None, None, 0, None, None, None, None, 0, None, None, None, None,
                                              None, None, C.byref(C.c_uint64()), C.byref(C.c_uint64()), None, 0, None) == -1


def test_contradicting_records_are_errors_and_write_nothing(engine, genome):
    r, want = records_on(genome, [("chrA1", "+", 10, 50), ("chrA2", "-", 90, 140), ("chrB1", "+", 0, 30), ("chrB2", "-", 200, 257)])
    assert call_bases(engine, genome, **r) == want
    off = r["rec_off"]
    cases_ = [dict(rec_off=np.array([off[0], off[2], off[1], off[3], off[4]], np.uint64)),         # descending offsets
              dict(rec_off=np.concatenate([off[:-1], [off[-1] - 1]]).astype(np.uint64)),          # the last record a byte short
              dict(rec_off=(off + np.uint64(1))),                                                 # not from 0
              dict(rec_hi=np.array([50, 140, 30, 258], np.uint32), rec_off=np.concatenate([off[:-1], [off[-1] + 1]]).astype(np.uint64)),
              dict(rec_lo=np.array([10, 141, 0, 200], np.uint32)),                                 # lo > hi (and the length)
              dict(rec_group=np.array([0, 1, 2, 4], np.uint32)), dict(group_cluster=np.array([0, 1, 2, 4], np.uint32)),
              dict(cl_entry=np.array([0, 1, 2, 4], np.uint32))]
    for change in cases_:
        call_bases(engine, genome, expect_error=True, **dict(r, **change))
    call_bases(engine, genome, expect_error=True, entry_base=[0, 1], **r)                          # parts that do not add up
    call_bases(engine, genome, expect_error=True, entry_len=genome["entry_len"][:3], **r)


# ------------------------------------------------------------------------------------------------ whole routes
def resident(engine, parts, tag):
    keys = ["precursor_world:%s:%d" % (tag, k) for k in range(len(parts))]
    for k, ix in zip(keys, parts):
        if k not in engine.libs:
            engine.add_library(k, ix, exact_dict=False)
    return keys


@pytest.mark.parametrize("w", WORLDS, ids=lambda w: w["name"])
def test_golden_worlds_byte_for_byte(engine, tmp_path, w):
    from mirge_amd import predict
    from tests.test_gpu_predict_features import world_inputs
    tables = {x["name"]: x for x in feature_cases.golden_worlds()}
    if w["name"] in tables:      # from the sorted table: the feature stage, then the precursors from what it left on the device
        t = tables[w["name"]]
        a = feature_cases.Arrays(t["table"], t["chromosomes"])
        rs, parts, trim, remap = world_inputs(engine, a)
        keys = resident(engine, parts, w["name"])
        stem = str(tmp_path / t["table_name"][:-len(SUFFIX)])
        feats = predict.cluster_features(engine, rs, a.counts, trim, remap, parts, stem, keep_device=True)
        assert open(stem + SUFFIX[:-4] + "_features.tsv").read() == w["features"]
        timings = {}
        got = predict.cluster_precursors(engine, feats, trim, parts, stem, timings=timings, parts_libs=keys)
        assert open(stem + SUFFIX[:-4] + "_features_precusor.fa").read() == w["precursors"]
        assert got["records"] == w["precursors"].count(">") == 2 * got["n_written"] and got["bytes"] == len(w["precursors"])
        if got["records"]:
            assert set(timings) >= {"device_ms", "download_ms", "write_s"}
        return
    a = cases.Arrays(w["features"], w["chromosomes"])
    parts, index = a.indexes()
    keys = resident(engine, parts, w["name"])
    d = Dev(engine)
    dev = dict(order=d.up(a.order, np.uint32), group_cluster=d.up(a.group_cluster, np.uint32), frame=d.up(a.frame, np.int32),
               valid=d.up(a.valid, np.uint8), n_sorted=a.n_groups, n_groups=a.n_groups)
    got = engine.predict_precursors(dev, a.cl, a.entry_len, keys)
    for k in ("rec_group", "rec_lo", "rec_hi", "rec_off"):
        assert list(got[k]) == list(a.rec[k]), k
    assert got["seq"] == a.rec["seq"] and got["n_written"] == a.n_groups
    path = str(tmp_path / "hand.fa")
    predict.write_precursors(path, parts, index, a.cl["entry"], a.group_cluster, got)
    assert open(path).read() == w["precursors"]


def test_predict_features_keeps_its_keys(engine):
    from tests.test_gpu_predict_features import world_inputs
    t = feature_cases.golden_worlds()[0]
    a = feature_cases.Arrays(t["table"], t["chromosomes"])
    rs, parts, trim, remap = world_inputs(engine, a)
    cl = dict(a.cl, kept=a.kept, kept_seq_off=a.kept_seq_off, kept_orig=a.kept_orig)
    host_groups = lambda g, lo, hi, c: None
    plain = engine.predict_features(rs, a.counts, remap["device"], cl, a.entry_len, a.entry_rank, host_groups)
    kept = engine.predict_features(rs, a.counts, remap["device"], cl, a.entry_len, a.entry_rank, host_groups, keep_device=True)
    also = engine.predict_features(rs, a.counts, remap["device"], cl, a.entry_len, a.entry_rank, host_groups, None, False)
    assert set(plain) == set(also) == FEATURE_KEYS and set(kept) == FEATURE_KEYS | {"device"}
    assert set(kept["device"]) >= {"order", "group_cluster", "frame", "valid", "cl_len", "n_sorted", "n_groups"}
    for k in ("order", "valid", "frame", "nb_flags"):
        assert np.array_equal(plain[k], kept[k])


def synthetic_genome(rng):
    from tests.test_gpu_predict_remap import extra_reads, twin_loci
    from tests.test_gpu_predict_trim import piles
    from tests.test_gpu_predict_trim import rand_seq as plain_seq
    names = ["chr1", "chr2", "scaffold_9"]
    texts = [plain_seq(rng, 20000) for _ in names]
    twin_loci(texts)
    return names, texts, piles(rng, texts, 300) + extra_reads(texts)


def test_map_and_cluster_with_precursors_equals_the_model(engine, oracle_lib, tmp_path):
    from mirge_amd import predict
    from mirge_amd.index import FmIndex
    from tests.test_gpu_predict_trim import REPEATS_TSV
    names, texts, reads = synthetic_genome(np.random.default_rng(48))
    genome_prefix = str(tmp_path / "syn_genome")
    FmIndex.build(names, texts).save(genome_prefix + ".mrgfm")
    reads = list(dict.fromkeys(reads))
    fa = tmp_path / "unmapped_mirna_s1.fa"
    fa.write_text("".join(">mir%d_%d\n%s\n" % (k + 5, 2 + k % 5, r) for k, r in enumerate(reads)))
    (tmp_path / "rep.tsv").write_text(REPEATS_TSV)
    feat, prec, shell = tmp_path / "feat", tmp_path / "prec", tmp_path / "shell"
    for d in (feat, prec, shell):
        d.mkdir()
    base = "unmapped_mirna_s1"
    trim = (str(tmp_path / "rep.tsv"), 24)
    cl0 = predict.map_and_cluster(engine, str(fa), genome_prefix, 3, 25, 14, str(feat / base), trim=trim, remap=True, features=True)
    cl = predict.map_and_cluster(engine, str(fa), genome_prefix, 3, 25, 14, str(prec / base), trim=trim, remap=True, features=True,
                                 precursors=True)
    new = base + SUFFIX[:-4] + "_features_precusor.fa"
    old = sorted(os.listdir(str(feat)))
    assert sorted(os.listdir(str(prec))) == sorted(old + [new])
    for fn in old:
        assert (feat / fn).read_bytes() == (prec / fn).read_bytes(), fn
    assert sorted(set(cl) - set(cl0)) == ["precursors"] and set(cl["features"]) == set(cl0["features"])
    want = model.run((prec / (base + SUFFIX[:-4] + "_features.tsv")).read_text(), dict(zip(names, texts)))
    assert (prec / new).read_text() == want
    assert cl["precursors"]["records"] == want.count(">") == 2 * cl["features"]["lines"] > 6 and cl["precursors"]["bytes"] == len(want)
    with pytest.raises(ValueError, match="precursors needs features"):
        predict.map_and_cluster(engine, str(fa), genome_prefix, 3, 25, 14, str(prec / "x"), trim=trim, remap=True, precursors=True)
    assert predict.main(["clusters", genome_prefix, str(fa), "-o", str(shell / base), "--trim", "--repeats", str(tmp_path / "rep.tsv"),
                         "-clc", "24", "--remap", "--features", "--precursors"]) == 0
    assert sorted(os.listdir(str(shell))) == sorted(os.listdir(str(prec)))
    assert (shell / new).read_bytes() == (prec / new).read_bytes()


def test_cli_novel_precursors_adds_one_file_per_sample(tmp_path_factory, native_lib, oracle_lib, tmp_path):
    from mirge_amd import cli
    from mirge_amd.index import FmIndex
    from tests import util
    from tests.test_gpu_predict_trim import REPEATS_TSV
    w = util.World(n_fixed=600, n_var=150)
    root = str(tmp_path_factory.mktemp("precursor_libs") / "libs")
    w.libs.write_layout(root, species="syn", db="miRBase")
    rng = np.random.default_rng(47)
    names, texts, novel = synthetic_genome(rng)
    fastqs = []
    for i, name in enumerate(("left.fastq", "right.fastq")):
        reads = list(w.reads[i::2][:300]) + [r for r in novel for _ in range(int(rng.choice([2, 3, 5])))]
        fastqs.append(str(tmp_path / name))
        with open(fastqs[-1], "w") as fh:
            fh.write("".join("@r%d\n%s\n+\n%s\n" % (k, r, "I" * len(r)) for k, r in enumerate(reads)))
    FmIndex.build(names, texts).save(os.path.join(root, "syn", "index.Libs", "syn_genome") + ".mrgfm")
    os.makedirs(os.path.join(root, "syn", "annotation.Libs"), exist_ok=True)
    with open(os.path.join(root, "syn", "annotation.Libs", "syn_genome_repeats.tsv"), "w") as fh:
        fh.write(REPEATS_TSV)
    res = cli.annotate_main(cli.build_parser().parse_args(
        ["annotate", "-s"] + fastqs + ["-lib", root, "-sp", "syn", "-o", str(tmp_path / "prec"), "--novel-precursors", "-clc", "24", "-sl", "18"]))
    out = os.path.join(res["outdir"], "unmapped_tmp")
    chromosomes = dict(zip(names, texts))
    for stem in ("left", "right"):
        sub = os.path.join(out, "unmapped_mirna_%s_tmp" % stem)
        table = "unmapped_mirna_" + stem + SUFFIX[:-4]
        assert {table + ".tsv", table + "_features.tsv", table + "_cluster.txt", table + "_features_precusor.fa"} <= set(os.listdir(sub))
        features = open(os.path.join(sub, table + "_features.tsv")).read()
        want = model.run(features, chromosomes)
        assert open(os.path.join(sub, table + "_features_precusor.fa")).read() == want and want.count(">") == 2 * (features.count("\n") - 1) > 0
