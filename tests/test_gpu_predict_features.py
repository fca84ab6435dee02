"""Predict mode's cluster feature table on the GPU (-m gpu): the row kernel against mirge_amd.a2i.local_pair, the group
stage against numpy, the tally and the neighbour step against the model (tests/predict_features_model.py) on hand-made
arrays with guard words behind every output; inconsistent arrays; the golden worlds of the reference through
predict.cluster_features byte for byte; predict.map_and_cluster(..., features=True) and `annotate --novel-features` end to
end against the model run over the table the same run wrote."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import predict_features_cases as cases
from tests import predict_features_model as model

pytestmark = pytest.mark.gpu

WORLDS = cases.golden_worlds()
GUARD = 64
SUFFIX = "_vs_representative_seq_modified_selected_sorted.tsv"
SIGNED = {np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}


@pytest.fixture(scope="module")
def engine(native_lib):
    from mirge_amd.engine import Engine
    eng = Engine(0)
    yield eng
    eng.close()


class Dev:
    """Device buffers with guard words behind the outputs."""

    def __init__(self, engine):
        import torch
        self.torch, self.engine, self.outs = torch, engine, []

    def up(self, a, dtype):
        a = np.array(a, dtype=dtype)          # (a copy: torch wants writable memory)
        if a.size == 0:
            a = np.zeros(1, dtype)
        return self.torch.from_numpy(a.view(SIGNED.get(a.dtype, a.dtype))).to(self.engine.device)

    def out(self, n, dtype):
        dtype = np.dtype(dtype)
        a = np.full(int(n) + GUARD, 0x5A, dtype=SIGNED.get(dtype, dtype))
        t = self.torch.from_numpy(a).to(self.engine.device)
        self.outs.append((t, int(n)))
        return t

    def tmp(self, n_rows):
        need = C.c_uint64()
        assert self.engine._lib.mrg_predict_feature_temp_bytes(int(n_rows), C.byref(need)) == 0
        return self.torch.empty(max(int(need.value), 64), dtype=self.torch.uint8, device=self.engine.device)

    def guards_intact(self):
        for t, n in self.outs:
            tail = t.cpu().numpy()[n:]
            assert tail.shape[0] == GUARD and (tail == 0x5A).all()
        return True


def host(t, n, dtype):
    return t.cpu().numpy()[:n].view(dtype)


def rand_seq(rng, L):
    return "".join("ACGT"[c] for c in rng.integers(0, 4, L))


# ------------------------------------------------------------------------------------------------ the row kernel
def align_pairs(engine, pairs):
    """mrg_predict_feature_align with one row, one group and one cluster per (cluster, read) pair: (status, diag, ident)."""
    from mirge_amd import pack
    d = Dev(engine)
    n = len(pairs)
    words, lens, nmask = pack.pack_reads([r for _, r in pairs])
    cseqs = [c for c, _ in pairs]
    soff = np.zeros(n + 1, np.uint64)
    np.cumsum([len(c) for c in cseqs], out=soff[1:])
    orig = np.frombuffer("".join(cseqs).encode(), dtype=np.uint8)
    ids = np.arange(n, dtype=np.uint32)
    t_ids, t_pass = d.up(ids, np.uint32), d.up(np.ones(n, np.uint8), np.uint8)
    t_words, t_lens = d.up(words.reshape(-1), np.uint64), d.up(lens, np.uint8)
    t_nmask = None if nmask is None else d.up(nmask.reshape(-1), np.uint64)
    t_soff, t_orig = d.up(soff, np.uint64), d.up(orig, np.uint8)
    cl_word, cl_len = d.out(n, np.uint64), d.out(n, np.uint8)
    status, diag, ident, ghost = d.out(n, np.uint8), d.out(n, np.int32), d.out(n, np.uint8), d.out(n, np.uint8)
    tmp = d.tmp(n)
    rc = engine._lib.mrg_predict_feature_align(
        engine._h, n, t_ids.data_ptr(), t_ids.data_ptr(), t_ids.data_ptr(), n, t_pass.data_ptr(), t_words.data_ptr(), t_lens.data_ptr(),
        None if t_nmask is None else t_nmask.data_ptr(), n, n, t_soff.data_ptr(), t_orig.data_ptr(), len(orig), cl_word.data_ptr(),
        cl_len.data_ptr(), status.data_ptr(), diag.data_ptr(), ident.data_ptr(), ghost.data_ptr(), tmp.data_ptr(), tmp.numel(),
        engine._stream_ptr())
    assert rc == 0 and d.guards_intact()
    st = host(status, n, np.uint8)
    assert (host(ghost, n, np.uint8) == (st >= 3)).all()
    return st, host(diag, n, np.int32), host(ident, n, np.uint8)


def expected_pair(cluster, read):
    """(kind, diag, ident) of a2i.local_pair: kind "ungapped", "gapped", "none" (no matching base) or "long" / "n"."""
    from mirge_amd.a2i import local_pair
    if len(cluster) > 32 or len(read) > 32 or set(cluster) - set("ACGT"):      # (not packable: status 3)
        return "long", 0, 0
    if "N" in read:
        return "n", 0, 0
    try:
        cpad, spad = local_pair(cluster, read)
    except ValueError:
        return "none", 0, 0
    if "-" in cpad.strip("-") or "-" in spad.strip("-"):
        return "gapped", 0, 0
    lead = lambda s: len(s) - len(s.lstrip("-"))
    return "ungapped", lead(spad) - lead(cpad), model.identity(cpad, spad)


def check_pairs(engine, pairs, must_settle=False):
    st, diag, ident = align_pairs(engine, pairs)
    kinds = {"long": 3, "n": 4, "gapped": 5, "none": 7}
    seen = {}
    for k, (c, r) in enumerate(pairs):
        kind, d, i = expected_pair(c, r)
        seen[kind] = seen.get(kind, 0) + 1
        if kind == "ungapped":
            assert st[k] in (0, 1, 6), (c, r, st[k])          # 6: a tie the settle rule leaves to the host
            if must_settle:
                assert st[k] in (0, 1), (c, r, st[k])
            if st[k] != 6:
                assert (diag[k], ident[k]) == (d, i), (c, r, st[k], diag[k], ident[k], d, i)
        else:
            assert st[k] == kinds[kind], (c, r, kind, st[k])
    return st, seen


def test_row_kernel_every_length_pair(engine):
    rng = np.random.default_rng(813)
    pairs = []
    for la in range(1, 33):
        for lb in range(1, 33):
            c = rand_seq(rng, la)
            if lb <= la and rng.random() < 0.6:          # a piece of the cluster, one base changed now and then
                at = int(rng.integers(0, la - lb + 1))
                r = c[at:at + lb]
                if lb > 6 and rng.random() < 0.5:
                    p = int(rng.integers(0, lb))
                    r = r[:p] + "ACGT"[("ACGT".index(r[p]) + 1) % 4] + r[p + 1:]
            elif rng.random() < 0.5:                       # overhanging both ends
                r = rand_seq(rng, 2) + c[:max(lb - 4, 0)] + rand_seq(rng, 2)
                r = (r + rand_seq(rng, lb))[:lb]
            else:
                r = rand_seq(rng, lb)
            pairs.append((c, r))
    st, seen = check_pairs(engine, pairs)
    assert seen["ungapped"] > 900 and (st == 0).sum() > 500 and (st == 1).sum() > 20


def test_row_kernel_planted_ties_gap_n_and_33(engine):
    rng = np.random.default_rng(814)
    unit = "ACGGTC"
    ties = [(unit * 4, unit * 3), (unit * 5, unit * 2), ("ACGT" * 6, "ACGT" * 3), ("A" * 20, "A" * 10), ("AC" * 12, "CA" * 6)]
    st, _ = check_pairs(engine, ties[:2], must_settle=True)
    assert (st == 1).all()
    st, _ = check_pairs(engine, ties[2:])         # (homopolymers and dinucleotide runs: settled, or left to the host)
    assert set(st) <= {1, 6}
    left, right = rand_seq(rng, 15), rand_seq(rng, 15)
    gapped = [(left + "G" + right, left + right), (left + right, left + "T" + right)]       # 30 matches - 20 beat 15 matches
    others = [(rand_seq(rng, 22), "ACGTACGTNACGTACGTAC"), (rand_seq(rng, 33), rand_seq(rng, 20)), (rand_seq(rng, 20), rand_seq(rng, 33)),
              ("ACGTACGTACGTNACGTACG", "ACGTACGTACGT"), ("AAAAAAAAAA", "CCCCCCCC")]
    st, seen = check_pairs(engine, gapped + others)
    assert list(st) == [5, 5, 4, 3, 3, 3, 7] and seen["gapped"] == 2


# ------------------------------------------------------------------------------------------------ the group stage
def call_groups(engine, row_read, row_cluster, counts, cl, soff, entry_len, expect_error=False):
    d = Dev(engine)
    T, n, K, E = len(row_read), len(counts), len(cl["entry"]), len(entry_len)
    ins = [d.up(row_read, np.uint32), d.up(row_cluster, np.uint32), d.up(counts, np.uint32), d.up(cl["entry"], np.uint32),
           d.up(cl["start"], np.uint32), d.up(cl["end"], np.uint32), d.up(soff, np.uint64), d.up(entry_len, np.uint32)]
    row_group, group_off, group_cluster = d.out(T, np.uint32), d.out(T + 1, np.uint32), d.out(T, np.uint32)
    group_sum, group_pass = d.out(T, np.uint64), d.out(T, np.uint8)
    tmp = d.tmp(T)
    G, P = C.c_uint64(77), C.c_uint64(77)
    rc = engine._lib.mrg_predict_feature_groups(
        engine._h, T, ins[0].data_ptr(), ins[1].data_ptr(), n, ins[2].data_ptr(), K, ins[3].data_ptr(), ins[4].data_ptr(), ins[5].data_ptr(),
        ins[6].data_ptr(), int(soff[-1]), E, ins[7].data_ptr(), row_group.data_ptr(), group_off.data_ptr(), group_cluster.data_ptr(),
        group_sum.data_ptr(), group_pass.data_ptr(), C.byref(G), C.byref(P), tmp.data_ptr(), tmp.numel(), engine._stream_ptr())
    assert d.guards_intact()
    if expect_error:
        assert rc == -1
        return None
    assert rc == 0
    G = int(G.value)
    return dict(G=G, P=int(P.value), row_group=host(row_group, T, np.uint32), group_off=host(group_off, G + 1 if T else 0, np.uint32),
                group_cluster=host(group_cluster, G, np.uint32), group_sum=host(group_sum, G, np.uint64), group_pass=host(group_pass, G, np.uint8))


def group_world(rng, runs, n_reads=50, big_counts=False):
    """Rows with the given run lengths, every run on a cluster of its own."""
    K = len(runs)
    row_cluster = np.repeat(np.arange(K, dtype=np.uint32), runs)
    row_read = rng.integers(0, n_reads, len(row_cluster)).astype(np.uint32)
    counts = (rng.integers(2 ** 31, 2 ** 32, n_reads) if big_counts else rng.integers(1, 6, n_reads)).astype(np.uint32)
    lens = rng.integers(18, 31, K)
    soff = np.zeros(K + 1, np.uint64)
    np.cumsum(lens, out=soff[1:])
    start = rng.integers(15, 30, K).astype(np.uint32)
    entry_len = np.array([100, 2 ** 31 - 1], dtype=np.uint32)
    entry = rng.integers(0, 2, K).astype(np.uint32)
    cl = dict(entry=entry, start=start, end=(start + lens - 1).astype(np.uint32))
    return row_read, row_cluster, counts, cl, soff, entry_len


def check_groups(engine, world):
    row_read, row_cluster, counts, cl, soff, entry_len = world
    got = call_groups(engine, *world)
    T = len(row_read)
    if T == 0:
        assert got["G"] == 0 and got["P"] == 0
        return got
    starts = np.flatnonzero(np.r_[True, row_cluster[1:] != row_cluster[:-1]])
    off = np.r_[starts, T].astype(np.uint32)
    assert got["G"] == len(starts) and (got["group_off"] == off).all() and (got["group_cluster"] == row_cluster[starts]).all()
    assert (got["row_group"] == np.repeat(np.arange(len(starts)), np.diff(off.astype(np.int64)))).all()
    sums = np.array([int(counts[row_read[a:b]].astype(np.uint64).sum()) for a, b in zip(off[:-1], off[1:])], dtype=np.uint64)
    assert (got["group_sum"] == sums).all()
    c = row_cluster[starts]
    want = (sums >= 10) & (np.diff(off.astype(np.int64)) >= 3) & (cl["start"][c] > 20) & \
        (cl["end"][c].astype(np.int64) < entry_len[cl["entry"][c]].astype(np.int64) - 20)
    assert (got["group_pass"] == want).all() and got["P"] == int(want.sum())
    return got


@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 4097])
def test_group_stage_row_counts(engine, n):
    rng = np.random.default_rng(900 + n)
    runs = []
    while sum(runs) < n:
        runs.append(min(int(rng.integers(1, 9)), n - sum(runs)))
    got = check_groups(engine, group_world(rng, runs))
    assert n < 63 or 0 < got["P"] < got["G"]


def test_group_stage_long_run_and_sums_past_2_32(engine):
    rng = np.random.default_rng(77)
    got = check_groups(engine, group_world(rng, [1, 5000, 2, 1, 300, 3], big_counts=True))
    assert int(got["group_sum"][1]) > 2 ** 32 * 1000


def test_group_stage_filter_edges(engine):
    # (count sum, members, start, end against an entry of 100) on the four edges
    cases_ = [(9, 3, 21, 79, 0), (10, 3, 21, 79, 1), (10, 2, 21, 79, 0), (10, 3, 20, 79, 0), (10, 3, 21, 80, 0), (10, 3, 21, 78, 1)]
    row_read, row_cluster, counts = [], [], []
    for k, (total, members, _, _, _) in enumerate(cases_):
        for m in range(members):
            row_cluster.append(k)
            row_read.append(len(counts))
            counts.append(total - (members - 1) if m == 0 else 1)
    start = np.array([c[2] for c in cases_], np.uint32)
    end = np.array([c[3] for c in cases_], np.uint32)
    soff = np.r_[0, np.cumsum(end.astype(np.int64) - start + 1)].astype(np.uint64)
    world = (np.array(row_read, np.uint32), np.array(row_cluster, np.uint32), np.array(counts, np.uint32),
             dict(entry=np.zeros(len(cases_), np.uint32), start=start, end=end), soff, np.array([100], np.uint32))
    got = check_groups(engine, world)
    assert list(got["group_pass"]) == [c[4] for c in cases_]


def test_group_stage_inconsistent_arrays_are_errors(engine):
    rng = np.random.default_rng(5)
    row_read, row_cluster, counts, cl, soff, entry_len = group_world(rng, [3, 4, 5, 6])
    bad_read = row_read.copy()
    bad_read[5] = len(counts)
    call_groups(engine, bad_read, row_cluster, counts, cl, soff, entry_len, expect_error=True)
    bad_cluster = row_cluster.copy()
    bad_cluster[7] = 4
    call_groups(engine, row_read, bad_cluster, counts, cl, soff, entry_len, expect_error=True)
    call_groups(engine, row_read, row_cluster, counts, dict(cl, end=cl["end"] + np.array([0, 1, 0, 0], np.uint32)), soff, entry_len, expect_error=True)
    call_groups(engine, row_read, row_cluster, counts, dict(cl, entry=np.array([0, 1, 2, 0], np.uint32)), soff, entry_len, expect_error=True)
    down = soff.copy()
    down[2] = down[1] - 1
    call_groups(engine, row_read, row_cluster, counts, cl, down, entry_len, expect_error=True)


# ------------------------------------------------------------------------------------------------ the tally
def frames_text(cseq, members):
    """(rows, H, T) of the ungapped frame of members [(read, diag, count)]."""
    H = max([0] + [-d for _, d, _ in members])
    T = max([0] + [d + len(r) - len(cseq) for r, d, _ in members])
    width = H + len(cseq) + T
    rows = ["-" * H + cseq + "-" * T]
    for r, d, _ in members:
        rows.append(("-" * (H + d) + r).ljust(width, "-"))
    return rows, H, T


def tally_groups(engine, groups, host_marked=()):
    """mrg_predict_feature_tally over groups [(cluster sequence, [(read, diag, count)])]: the arrays it leaves."""
    from mirge_amd import pack
    d = Dev(engine)
    reads, counts, diag, ident, off = [], [], [], [], [0]
    for cseq, members in groups:
        for r, dg, cnt in members:
            reads.append(r)
            counts.append(cnt)
            diag.append(dg)
            ident.append(sum(1 for i, ch in enumerate(r) if 0 <= dg + i < len(cseq) and cseq[dg + i] == ch))
        off.append(len(reads))
    G, T = len(groups), len(reads)
    words, lens, _ = pack.pack_reads(reads)
    ghost = np.zeros(G, np.uint8)
    ghost[list(host_marked)] = 1
    ins = [d.up(off, np.uint32), d.up(np.arange(G), np.uint32), d.up(np.ones(G, np.uint8), np.uint8), d.up(ghost, np.uint8),
           d.up(np.arange(T), np.uint32), d.up(diag, np.int32), d.up(ident, np.uint8), d.up(words.reshape(-1), np.uint64), d.up(lens, np.uint8),
           d.up(counts, np.uint32), d.up([len(c) for c, _ in groups], np.uint8)]
    valid, frame, exact, nine = d.out(G, np.uint8), d.out(4 * G, np.int32), d.out(G, np.uint64), d.out(45 * G, np.uint64)
    rc = engine._lib.mrg_predict_feature_tally(
        engine._h, G, ins[0].data_ptr(), ins[1].data_ptr(), ins[2].data_ptr(), ins[3].data_ptr(), T, ins[4].data_ptr(), ins[5].data_ptr(),
        ins[6].data_ptr(), ins[7].data_ptr(), ins[8].data_ptr(), T, ins[9].data_ptr(), G, ins[10].data_ptr(), valid.data_ptr(),
        frame.data_ptr(), exact.data_ptr(), nine.data_ptr(), engine._stream_ptr())
    assert rc == 0
    d.torch.cuda.synchronize()
    assert d.guards_intact()
    return host(valid, G, np.uint8), host(frame, 4 * G, np.int32).reshape(G, 4), host(exact, G, np.uint64), host(nine, 45 * G, np.uint64).reshape(G, 45)


def check_tally(engine, groups):
    valid, frame, exact, nine = tally_groups(engine, groups)
    for g, (cseq, members) in enumerate(groups):
        rows, H, T = frames_text(cseq, members)
        counts = [c for _, _, c in members]
        _, _, _, head, tail = model.locate(rows, counts)
        assert (frame[g][0], frame[g][1]) == (H, T), g
        assert valid[g] == (head is not None), g
        if head is None:
            assert not nine[g].any()
            continue
        assert (frame[g][2], frame[g][3]) == (head, tail), (g, frame[g], head, tail)
        assert exact[g] == sum(c for (r, dg, c), row in zip(members, rows[1:]) if model.identity(rows[0], row) == len(r))
        cols, pad_h, pad_t = model.feature_columns(len(rows[0]), head, tail)
        padded = ["-" * pad_h + r + "-" * pad_t for r in rows]
        want = []
        for x in cols:
            t = model.tallies(padded, counts, x + pad_h)
            want += [t[b] for b in model.BASES] + [t["-"]]
        assert list(nine[g]) == want, (g, list(nine[g]), want)
    return valid, frame


def mutate(s, i, step=1):
    return s[:i] + "ACGT"[("ACGT".index(s[i]) + step) % 4] + s[i + 1:]


def test_tally_frames_of_1_64_65_and_94_columns(engine):
    rng = np.random.default_rng(31)
    c32 = rand_seq(rng, 32)
    wide = lambda H, T: (c32, [(c32, 0, 20), (rand_seq(rng, H) + c32[:32 - H], -H, 3), (c32[T:] + rand_seq(rng, T), T, 2),
                               (c32[4:30], 4, 1)])
    groups = [("A", [("A", 0, 5), ("A", 0, 4), ("C", 0, 1)]), wide(16, 16), wide(17, 16), wide(31, 31), wide(31, 0), wide(0, 31)]
    _, frame = check_tally(engine, groups)
    assert [int(f[0] + f[1]) + len(g[0]) for f, g in zip(frame, groups)] == [1, 64, 65, 94, 63, 63]


def test_tally_head_tail_paddings_and_ratio_edges(engine):
    rng = np.random.default_rng(32)
    groups = []
    for head in range(0, 6):                      # head 0 .. 5 and tailAdd 0 .. 8: every padding case
        for tail_add in (0, 1, 5, 6, 7, 8):
            c = rand_seq(rng, 24)
            groups.append((c, [(c[head:24 - tail_add], head, 12), (c, 0, 1), (c[1:], 1, 1)]))
    c = rand_seq(rng, 22)
    groups.append((c, [(c, 0, 12), (mutate(c, 0), 0, 2), (mutate(c, 0, 2), 0, 1)]))                 # 12 / 15 = 4 / 5
    groups.append((c, [(c, 0, 14), (mutate(c, 0), 0, 2), (mutate(c, 0), 0, 2)]))                    # 14 / 18 = 7 / 9
    groups.append((c, [(c, 0, 8), (mutate(c, 21), 0, 1), (mutate(c, 21, 2), 0, 1)]))                # 8 / 10
    groups.append((c, [(c, 0, 5), (mutate(c, 10, 2), 0, 5), (c[11:], 11, 1)]))                      # a tie of two bases
    groups.append((c, [(c[0:8], 0, 4), (c[6:14], 6, 4), (c[12:20], 12, 4)]))                        # no stable column
    groups.append((c, [(c, 0, 2 ** 32 - 1)] * 4 + [(mutate(c, 3), 0, 2 ** 32 - 1)]))                # 4 / 5 of a sum past 2^32
    groups.append((c, [(c, 0, 1)] * 300 + [(c[2:], 2, 7)] * 70))                                    # more than 64 members, twice over
    valid, frame = check_tally(engine, groups)
    assert list(valid[-7:]) == [1, 1, 1, 1, 0, 1, 1] and frame[-6][2] == 1 and frame[-7][2] == 0


def test_tally_leaves_host_marked_groups_alone(engine):
    c = "ACGTTGCAAGGCTAGCTAGGAT"
    groups = [(c, [(c, 0, 8), (c[1:], 1, 1), (c[2:], 2, 1)])] * 3
    valid, frame, exact, nine = tally_groups(engine, groups, host_marked=[1])
    assert list(valid) == [1, 0, 1] and not frame[1].any() and exact[1] == 0 and not nine[1].any()


# ------------------------------------------------------------------------------------------------ the neighbour step
def call_neighbors(engine, group_cluster, valid, frame, cl, kept, entry_rank, expect_error=False):
    d = Dev(engine)
    G, K, E = len(group_cluster), len(kept), len(entry_rank)
    ins = [d.up(group_cluster, np.uint32), d.up(valid, np.uint8), d.up(np.asarray(frame).reshape(-1), np.int32), d.up(cl["entry"], np.uint32),
           d.up(cl["strand"], np.uint8), d.up(cl["start"], np.uint32), d.up(cl["end"], np.uint32), d.up(kept, np.uint32),
           d.up(entry_rank, np.uint32)]
    order, nb_t, nb_up, nb_down, nb_flags = d.out(G, np.uint32), d.out(G, np.uint32), d.out(G, np.int64), d.out(G, np.int64), d.out(G, np.uint8)
    tmp = d.tmp(G)
    S = C.c_uint64(77)
    rc = engine._lib.mrg_predict_feature_neighbors(
        engine._h, G, ins[0].data_ptr(), ins[1].data_ptr(), ins[2].data_ptr(), K, ins[3].data_ptr(), ins[4].data_ptr(), ins[5].data_ptr(),
        ins[6].data_ptr(), ins[7].data_ptr(), E, ins[8].data_ptr(), order.data_ptr(), nb_t.data_ptr(), nb_up.data_ptr(), nb_down.data_ptr(),
        nb_flags.data_ptr(), C.byref(S), tmp.data_ptr(), tmp.numel(), engine._stream_ptr())
    assert d.guards_intact()
    if expect_error:
        assert rc == -1
        return None
    assert rc == 0
    S = int(S.value)
    return host(order, G, np.uint32)[:S], host(nb_t, G, np.uint32), host(nb_up, G, np.int64), host(nb_down, G, np.int64), host(nb_flags, G, np.uint8)


def neighbor_world(rng, per_chrom):
    """Groups on chromosomes with the given group counts; gaps drawn around the four edges, equal starts among them."""
    names = ["chr%d" % k for k in (1, 10, 2, 21, 3, 4, 5)][:len(per_chrom)]
    rank = np.zeros(len(names), np.uint32)
    for k, nm in enumerate(sorted(names)):
        rank[names.index(nm)] = k
    entry, strand, start, end, frames, valid = [], [], [], [], [], []
    for e, n in enumerate(per_chrom):
        at = 30
        for _ in range(n + 1):                     # one more group than counted: it has no stable column
            L = int(rng.integers(18, 31))
            entry.append(e)
            strand.append(int(rng.integers(0, 2)))
            start.append(at)
            end.append(at + L - 1)
            H, T = int(rng.integers(0, 4)), int(rng.integers(0, 4))
            head = int(rng.integers(0, 5))
            tail = -1 - int(rng.integers(0, 7))
            frames.append((H, T, head, tail))
            valid.append(1)
            gap = int(rng.choice([8, 9, 44, 45, 0, -5, 20, 300]))
            at = at if rng.random() < 0.15 else end[-1] + 1 + gap + int(rng.integers(0, 3))
        valid[-1] = 0
    K = len(entry)
    perm = rng.permutation(K)                      # the groups in cluster-number order, not in coordinate order
    kept = (200 + rng.permutation(5000)[:K]).astype(np.uint32)
    kept[:min(K, 4)] = [8, 9, 98, 99][:min(K, 4)]  # numbers 9, 10, 99, 100: the digits' byte order is not the numbers'
    cl = dict(entry=np.array(entry, np.uint32)[perm], strand=np.array(strand, np.uint8)[perm], start=np.array(start, np.uint32)[perm],
              end=np.array(end, np.uint32)[perm])
    return names, rank, cl, kept, np.array(frames, np.int32)[perm], np.array(valid, np.uint8)[perm]


@pytest.mark.parametrize("per_chrom", [[0], [1], [2], [3, 0, 5], [4, 1, 2, 5, 3, 0, 5]], ids=lambda p: "-".join(map(str, p)))
def test_neighbors_against_the_model(engine, per_chrom):
    from tests import predict_remap_model as prm
    rng = np.random.default_rng(sum(per_chrom) + 10 * len(per_chrom))
    names, rank, cl, kept, frames, valid = neighbor_world(rng, per_chrom)
    G = len(kept)
    order, nb_t, nb_up, nb_down, nb_flags = call_neighbors(engine, np.arange(G), valid, frames, cl, kept, rank)
    want_order = sorted([g for g in range(G) if valid[g]], key=lambda g: (names[cl["entry"][g]], int(cl["start"][g]), int(cl["end"][g]),
                                                                         prm.name_key(int(kept[g]) + 1)))
    assert list(order) == want_order and len(order) == sum(per_chrom)
    seen_states = set()
    for e in range(len(names)):
        gs = [g for g in want_order if cl["entry"][g] == e]
        ivs = [(int(cl["start"][g]) + int(frames[g][2]) - int(frames[g][0]), int(cl["end"][g]) + 1 + int(frames[g][3]) + int(frames[g][1])) for g in gs]
        strands = ["-" if cl["strand"][g] else "+" for g in gs]
        for t, g in enumerate(gs):
            state, up, down = model.neighbor(t, ivs, strands)
            seen_states.add(state)
            assert nb_t[g] == t
            assert nb_flags[g] == ((1 if up is None else 0) | (2 if down is None else 0) | (cases.STATE[state] << 2)), (g, state, up, down)
            assert up is None or nb_up[g] == up
            assert down is None or nb_down[g] == down
    if sum(per_chrom) > 20:
        assert seen_states == {"Good", "Null", "Bad"}


def test_neighbors_distance_edges_and_strands(engine):
    # five groups 8, 9, 44 and 45 apart on +, then a chromosome with a - neighbour 20 away
    start, end, strand, entry = [], [], [], []
    at = 30
    for gap in (8, 9, 44, 45, None):
        start.append(at)
        end.append(at + 21)
        strand.append(0)
        entry.append(0)
        at += 22 + (gap or 0)
    start += [30, 72]
    end += [51, 93]
    strand += [0, 1]
    entry += [1, 1]
    G = len(start)
    cl = dict(entry=np.array(entry, np.uint32), strand=np.array(strand, np.uint8), start=np.array(start, np.uint32), end=np.array(end, np.uint32))
    frames = np.tile(np.array([0, 0, 0, -1], np.int32), (G, 1))
    order, nb_t, nb_up, nb_down, nb_flags = call_neighbors(engine, np.arange(G), np.ones(G, np.uint8), frames, cl, np.arange(G), np.array([0, 1]))
    assert list(order) == list(range(G)) and list(nb_t) == [0, 1, 2, 3, 4, 0, 1]
    assert list(nb_down[:4]) == [8, 9, 44, 45] and list(nb_up[1:5]) == [8, 9, 44, 45] and nb_down[5] == 20
    states = [f >> 2 for f in nb_flags]
    assert states == [2, 1, 1, 1, 0, 2, 2]                  # Bad, Good, Good, Good (44 upstream), Null; unequal strands: Bad
    assert [f & 3 for f in nb_flags] == [1, 0, 0, 0, 2, 1, 2]


def test_neighbors_inconsistent_arrays_are_errors(engine):
    rng = np.random.default_rng(3)
    names, rank, cl, kept, frames, valid = neighbor_world(rng, [3, 2])
    G = len(kept)
    bad = np.arange(G)
    bad[2] = G
    call_neighbors(engine, bad, valid, frames, cl, kept, rank, expect_error=True)
    call_neighbors(engine, np.arange(G), np.ones(G, np.uint8), frames, dict(cl, entry=cl["entry"] + 5), kept, rank, expect_error=True)


# ------------------------------------------------------------------------------------------------ whole routes
def world_inputs(engine, a):
    """A golden world's arrays as cluster_features takes them."""
    import torch
    from mirge_amd.engine import ReadSet
    words, lens, nmask = a.packed()
    rs = ReadSet(words, lens, nmask, device=engine.device)
    parts, index = a.indexes()
    trim = dict(kept=a.kept, kept_seq_off=a.kept_seq_off, kept_orig=a.kept_orig, clusters=a.cl)
    up = lambda x: torch.from_numpy(x.view(np.int32)).to(engine.device)
    zeros = np.zeros(len(a.row_read), np.uint8)
    remap = dict(n_rows=len(a.row_read), rows=(a.row_read, a.row_cluster, zeros.astype(np.uint32), zeros, zeros),
                 device=(up(a.row_read), up(a.row_cluster)), index=index)
    return rs, parts, trim, remap


@pytest.mark.parametrize("w", WORLDS, ids=lambda w: w["name"])
def test_golden_worlds_through_cluster_features(engine, tmp_path, w):
    from mirge_amd import predict
    a = cases.Arrays(w["table"], w["chromosomes"])
    exp = a.expected(w["table"])
    rs, parts, trim, remap = world_inputs(engine, a)
    stem = str(tmp_path / w["table_name"][:-len(SUFFIX)])
    timings = {}
    got = predict.cluster_features(engine, rs, a.counts, trim, remap, parts, stem, timings=timings)
    assert open(stem + SUFFIX[:-4] + "_features.tsv").read() == w["features"]
    assert open(stem + SUFFIX[:-4] + "_cluster.txt").read() == w["cluster"]
    info = exp["info"]
    assert (got["seen"], got["passed"], got["written"]) == (info["seen"], info["passed"], w["cluster"].count("Cluster Name: "))
    assert got["lines"] == max(w["features"].count("\n") - 1, 0)
    assert (got["group_sum"] == exp["group_sum"]).all() and (got["group_pass"] == exp["group_pass"]).all()
    assert (got["valid"] == exp["valid"]).all() and list(got["order"]) == list(exp["order"])
    ok = got["valid"] != 0
    assert (got["frame"][ok] == exp["frame"][ok]).all() and (got["nine"][ok] == exp["nine"][ok]).all() and (got["exact"][ok] == exp["exact"][ok]).all()
    if w["name"] == "main":
        assert got["host_groups"] == 1 and got["row_status_counts"][4] == 1 and got["row_status_counts"][1] >= 1   # the N; a settled tie
        assert got["row_status_counts"][2] == sum(1 for g in a.row_group if not exp["group_pass"][g])
        assert set(timings) >= {"device_ms", "download_ms", "host_s", "write_s"}


def test_map_and_cluster_with_features_equals_the_model(engine, oracle_lib, tmp_path):
    from mirge_amd import predict
    from mirge_amd.index import FmIndex
    from tests.test_gpu_predict_remap import extra_reads, twin_loci
    from tests.test_gpu_predict_trim import REPEATS_TSV, piles
    from tests.test_gpu_predict_trim import rand_seq as plain_seq
    rng = np.random.default_rng(48)
    names = ["chr1", "chr2", "scaffold_9"]
    texts = [plain_seq(rng, 20000) for _ in names]
    twin_loci(texts)
    genome = str(tmp_path / "syn_genome")
    FmIndex.build(names, texts).save(genome + ".mrgfm")
    reads = list(dict.fromkeys(piles(rng, texts, 300) + extra_reads(texts)))
    fa = tmp_path / "unmapped_mirna_s1.fa"
    fa.write_text("".join(">mir%d_%d\n%s\n" % (k + 5, 2 + k % 5, r) for k, r in enumerate(reads)))
    (tmp_path / "rep.tsv").write_text(REPEATS_TSV)
    mapped, feat = tmp_path / "mapped", tmp_path / "feat"
    mapped.mkdir()
    feat.mkdir()
    base = "unmapped_mirna_s1"
    cl0 = predict.map_and_cluster(engine, str(fa), genome, 3, 25, 14, str(mapped / base), trim=(str(tmp_path / "rep.tsv"), 24), remap=True)
    libs = dict(engine.libs)
    cl = predict.map_and_cluster(engine, str(fa), genome, 3, 25, 14, str(feat / base), trim=(str(tmp_path / "rep.tsv"), 24), remap=True,
                                 features=True)
    assert engine.libs == libs
    old = sorted(os.listdir(str(mapped)))
    new = [base + SUFFIX[:-4] + "_features.tsv", base + SUFFIX[:-4] + "_cluster.txt"]
    assert sorted(os.listdir(str(feat))) == sorted(old + new)
    for fn in old:
        assert (mapped / fn).read_bytes() == (feat / fn).read_bytes(), fn
    assert sorted(set(cl) - set(cl0)) == ["features"] and "device" not in cl["remap"] and "index" not in cl["remap"]
    chromosomes = dict(zip(names, texts))
    want_f, want_c, info = model.run((feat / (base + SUFFIX)).read_text(), chromosomes, base + SUFFIX)
    assert (feat / new[0]).read_text() == want_f
    assert (feat / new[1]).read_text() == want_c
    f = cl["features"]
    assert (f["seen"], f["passed"]) == (info["seen"], info["passed"]) and f["lines"] == want_f.count("\n") - 1 > 3
    with pytest.raises(ValueError, match="features needs remap"):
        predict.map_and_cluster(engine, str(fa), genome, 3, 25, 14, str(feat / "x"), trim=(str(tmp_path / "rep.tsv"), 24), features=True)
    shell = tmp_path / "shell"
    shell.mkdir()
    assert predict.main(["clusters", genome, str(fa), "-o", str(shell / base), "--trim", "--repeats", str(tmp_path / "rep.tsv"),
                         "-clc", "24", "--remap", "--features"]) == 0
    for fn in new:
        assert (shell / fn).read_bytes() == (feat / fn).read_bytes()


def test_cli_novel_features_adds_two_files_per_sample(tmp_path_factory, native_lib, oracle_lib, tmp_path):
    from mirge_amd import cli
    from mirge_amd.index import FmIndex
    from tests import util
    from tests.test_gpu_predict_remap import extra_reads, twin_loci
    from tests.test_gpu_predict_trim import REPEATS_TSV, piles
    from tests.test_gpu_predict_trim import rand_seq as plain_seq
    w = util.World(n_fixed=600, n_var=150)
    root = str(tmp_path_factory.mktemp("feature_libs") / "libs")
    w.libs.write_layout(root, species="syn", db="miRBase")
    rng = np.random.default_rng(47)
    names = ["chr1", "chr2", "scaffold_9"]
    texts = [plain_seq(rng, 20000) for _ in names]
    twin_loci(texts)
    novel = piles(rng, texts, 300) + extra_reads(texts)
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

    def annotate(out, *extra):
        res = cli.annotate_main(cli.build_parser().parse_args(
            ["annotate", "-s"] + fastqs + ["-lib", root, "-sp", "syn", "-o", str(out)] + list(extra)))
        return os.path.join(res["outdir"], "unmapped_tmp")
    before = annotate(tmp_path / "map", "--novel-map", "-clc", "24", "-sl", "18")
    after = annotate(tmp_path / "feat", "--novel-features", "-clc", "24", "-sl", "18")
    chromosomes = dict(zip(names, texts))
    for stem in ("left", "right"):
        sub = "unmapped_mirna_%s_tmp" % stem
        base = "unmapped_mirna_" + stem
        old = sorted(os.listdir(os.path.join(before, sub)))
        new = [base + SUFFIX[:-4] + "_features.tsv", base + SUFFIX[:-4] + "_cluster.txt"]
        assert sorted(os.listdir(os.path.join(after, sub))) == sorted(old + new)
        for fn in old:
            assert open(os.path.join(before, sub, fn), "rb").read() == open(os.path.join(after, sub, fn), "rb").read(), fn
        want_f, want_c, info = model.run(open(os.path.join(after, sub, base + SUFFIX)).read(), chromosomes, base + SUFFIX)
        assert open(os.path.join(after, sub, new[0])).read() == want_f and info["passed"] > 0
        assert open(os.path.join(after, sub, new[1])).read() == want_c
