"""Predict mode's screening of the folded candidates on the GPU (-m gpu): mrg_predict_screen_candidates / _prune / _features /
_select on the reference's own cases (tests/golden/predict_screen.json) and on hand-made arrays against the model
(tests/predict_screen_model.py), with guard words behind every output -- candidate counts around the four waves of a
workgroup, lengths 1 .. 257, the cases left to the host counted exactly, contradicting arrays --, the golden worlds end to end
through predict.screen_precursors byte for byte, and predict.map_and_cluster(..., screen=True), `predict clusters --screen` and
`annotate --novel-screen --fold-cmd` against the model run over the files the same run wrote, with the fold command counted."""
import ctypes as C
import os
import stat
import sys

import numpy as np
import pytest

from tests import predict_screen_cases as cases
from tests import predict_screen_model as model

pytestmark = pytest.mark.gpu

GOLD = cases.golden()
WORLDS, CASES = GOLD["worlds"], GOLD["cases"]
GUARD = 64
NO = cases.NO
SUFFIX = "_vs_representative_seq_modified_selected_sorted"
SIGNED = {np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}
HOST_CASES = 24      # the fixture's: 8 of length 257, 16 with ten or more stems or hairpins
WAVES = 4            # candidates a workgroup


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
        if isinstance(a, (bytes, bytearray)):
            a = np.frombuffer(bytes(a), dtype=np.uint8)
        a = np.array(a, dtype=dtype)
        if a.size == 0:
            a = np.zeros(1, dtype)
        return self.torch.from_numpy(a.reshape(-1).view(SIGNED.get(a.dtype, a.dtype))).to(self.engine.device)

    def out(self, n, dtype):
        dtype = np.dtype(dtype)
        a = np.full(int(n) + GUARD, 0x5A, dtype=SIGNED.get(dtype, dtype))
        t = self.torch.from_numpy(a).to(self.engine.device)
        self.outs.append((t, int(n)))
        return t

    def tmp(self, n_cand):
        need = C.c_uint64()
        assert self.engine._lib.mrg_predict_screen_temp_bytes(int(n_cand), C.byref(need)) == 0
        return self.torch.empty(max(int(need.value), 64), dtype=self.torch.uint8, device=self.engine.device)

    def guards_intact(self):
        for t, n in self.outs:
            tail = t.cpu().numpy()[n:]
            assert tail.shape[0] == GUARD and (tail == 0x5A).all()
        return True


def host(t, n, dtype):
    return t.cpu().numpy()[:n].view(dtype)


def error(engine):
    return (engine._lib.mrg_last_error() or b"").decode()


def call_candidates(engine, line_group, flags, up, down, expect_error=None):
    d = Dev(engine)
    n, G = len(line_group), len(flags)
    ins = [d.up(line_group, np.uint32), d.up(flags, np.uint8), d.up(up, np.int64), d.up(down, np.int64)]
    cand_n, cand_rec, cand_mir = d.out(n, np.uint8), d.out(4 * n, np.uint32), d.out(8 * n, np.uint32)
    tmp = d.tmp(0)
    p = lambda t: t.data_ptr()
    rc = engine._lib.mrg_predict_screen_candidates(engine._h, n, p(ins[0]), G, p(ins[1]), p(ins[2]), p(ins[3]), p(cand_n), p(cand_rec),
                                                   p(cand_mir), p(tmp), tmp.numel(), engine._stream_ptr())
    assert d.guards_intact()
    if expect_error is not None:
        assert rc == -1 and expect_error in error(engine), error(engine)
        return None
    assert rc == 0, error(engine)
    return host(cand_n, n, np.uint8), host(cand_rec, 4 * n, np.uint32), host(cand_mir, 8 * n, np.uint32).reshape(-1, 2)


def call_prune(engine, cand_rec, cand_mir, records, mirnas, expect_error=None, rec_off=None, cap=None):
    """records = [(sequence, structure)], mirnas = [str]."""
    d = Dev(engine)
    n = len(cand_rec)
    off, seq = cases.blob([r[0] for r in records])
    structure = cases.blob([r[1] for r in records])[1]
    moff, mir = cases.blob(mirnas)
    if rec_off is not None:
        off = np.array(rec_off, np.uint64)
    ins = [d.up(cand_rec, np.uint32), d.up(np.array(cand_mir, np.uint32).reshape(-1), np.uint32), d.up(off, np.uint64), d.up(seq, np.uint8),
           d.up(structure, np.uint8), d.up(moff, np.uint64), d.up(mir, np.uint8)]
    cap = 256 * n if cap is None else cap
    status, lo, hi, poff, pruned = d.out(n, np.uint8), d.out(n, np.uint32), d.out(n, np.uint32), d.out(n + 1, np.uint64), d.out(cap, np.uint8)
    tmp = d.tmp(n)
    total = C.c_uint64(99)
    p = lambda t: t.data_ptr()
    rc = engine._lib.mrg_predict_screen_prune(engine._h, n, p(ins[0]), p(ins[1]), len(records), p(ins[2]), p(ins[3]), p(ins[4]), len(seq),
                                              len(mirnas), p(ins[5]), p(ins[6]), len(mir), 15, p(status), p(lo), p(hi), p(poff), p(pruned), cap,
                                              C.byref(total), p(tmp), tmp.numel(), engine._stream_ptr())
    assert d.guards_intact()
    if expect_error is not None:
        assert rc == -1 and total.value == 0 and expect_error in error(engine), error(engine)
        return None
    assert rc == 0, error(engine)
    total = int(total.value)
    return dict(status=host(status, n, np.uint8), lo=host(lo, n, np.uint32), hi=host(hi, n, np.uint32), off=host(poff, n + 1, np.uint64),
                pruned=host(pruned, total, np.uint8).tobytes())


def call_features(engine, status, cand_mir, pruned, mirnas, expect_error=None, p_off=None):
    """pruned = [(sequence, structure)] per candidate."""
    d = Dev(engine)
    n = len(status)
    off, seq = cases.blob([r[0] for r in pruned])
    structure = cases.blob([r[1] for r in pruned])[1]
    moff, mir = cases.blob(mirnas)
    if p_off is not None:
        off = np.array(p_off, np.uint64)
    ins = [d.up(status, np.uint8), d.up(np.array(cand_mir, np.uint32).reshape(-1), np.uint32), d.up(off, np.uint64), d.up(seq, np.uint8),
           d.up(structure, np.uint8), d.up(moff, np.uint64), d.up(mir, np.uint8)]
    feat = d.out(16 * n, np.int32)
    tmp = d.tmp(n)
    p = lambda t: t.data_ptr()
    rc = engine._lib.mrg_predict_screen_features(engine._h, n, p(ins[0]), p(ins[1]), p(ins[2]), p(ins[3]), p(ins[4]), len(seq), len(mirnas),
                                                 p(ins[5]), p(ins[6]), len(mir), p(feat), p(tmp), tmp.numel(), engine._stream_ptr())
    assert d.guards_intact()
    if expect_error is not None:
        assert rc == -1 and expect_error in error(engine), error(engine)
        return None
    assert rc == 0, error(engine)
    return host(feat, 16 * n, np.int32).reshape(n, 16)


def call_select(engine, cand_n, cand_rec, rec_mfe, feat, expect_error=None, n_rec=None):
    d = Dev(engine)
    n = len(cand_n)
    ins = [d.up(cand_n, np.uint8), d.up(cand_rec, np.uint32), d.up(rec_mfe, np.float64), d.up(np.array(feat, np.int32).reshape(-1), np.int32)]
    best = d.out(n, np.int32)
    tmp = d.tmp(0)
    p = lambda t: t.data_ptr()
    rc = engine._lib.mrg_predict_screen_select(engine._h, n, p(ins[0]), p(ins[1]), len(rec_mfe) if n_rec is None else n_rec, p(ins[2]), p(ins[3]),
                                               15, p(best), p(tmp), tmp.numel(), engine._stream_ptr())
    assert d.guards_intact()
    if expect_error is not None:
        assert rc == -1 and expect_error in error(engine), error(engine)
        return None
    assert rc == 0, error(engine)
    return host(best, n, np.int32)


def case_arrays(which):
    """The fixture's cases `which` as one record and one candidate each, their miRNAs in one list."""
    records, mirnas, cand_mir = [], [], []
    for seq, structure, mirs, _, _ in which:
        records.append((seq, structure))
        cand_mir.append([len(mirnas), len(mirnas) + 1 if len(mirs) == 2 else NO])
        mirnas.extend(mirs)
    return records, mirnas, np.array(cand_mir, np.uint32).reshape(-1, 2)


def flags_of(states, up, down):
    """nb_flags as mrg_predict_feature_neighbors leaves them, from a feature file's three columns."""
    code = {"Good": 1, "Bad": 2}
    return np.array([(u == 10000) | ((d == 10000) << 1) | (code.get(s, 0) << 2) for s, u, d in zip(states, up, down)], np.uint8)


# ------------------------------------------------------------------------------------------------------- candidates
@pytest.mark.parametrize("w", WORLDS, ids=lambda w: w["name"])
def test_candidates_of_the_worlds(engine, w):
    a = cases.world_arrays(w)
    n = a["n"]
    order = np.arange(n, dtype=np.uint32)[::-1].copy()           # line i is group n - 1 - i: the kernel goes through line_group
    flags = flags_of(a["states"], a["up"], a["down"])
    up = np.where(np.array(a["up"], np.int64) == 10000, -7, np.array(a["up"], np.int64))     # (a `None` distance is not read)
    down = np.where(np.array(a["down"], np.int64) == 10000, -7, np.array(a["down"], np.int64))
    pick = lambda x: np.array(x)[::-1].copy() if n else np.array(x)
    cand_n, cand_rec, cand_mir = call_candidates(engine, order, pick(flags), pick(up), pick(down))
    assert cand_n.tolist() == a["cand_n"].tolist() and cand_rec.tolist() == a["cand_rec"].tolist()
    assert cand_mir.tolist() == a["cand_mir"].tolist()


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_candidates_around_the_block_size(engine, n):
    rng = np.random.default_rng(n)
    rows = []
    for i in range(n):
        kind = int(rng.integers(0, 5)) if 0 < i < n - 1 else 0
        near, far = int(rng.integers(9, 45)), int(rng.choice([0, 8, 45, 10000]))
        state, up, down = [("Null", far, near), ("Bad", near, near), ("Good", far, near), ("Good", near, near), ("Good", near, far)][kind]
        rows.append(("line\n", "c%d" % i, "ACGU", state, up, down))
    want = model.candidates(rows)
    flags = flags_of([r[3] for r in rows], [r[4] for r in rows], [r[5] for r in rows])
    cand_n, cand_rec, cand_mir = call_candidates(engine, np.arange(n), flags, [r[4] for r in rows], [r[5] for r in rows])
    for i, (recs, mirs) in enumerate(want):
        assert cand_n[i] == len(recs) and cand_rec[4 * i:4 * i + 4].tolist() == recs + [NO] * (4 - len(recs))
        for k in range(4):
            assert cand_mir[4 * i + k].tolist() == ((mirs[k] + [NO])[:2] if k < len(recs) else [NO, NO])


def test_candidates_refuse_what_the_reference_dies_of(engine):
    assert call_candidates(engine, [], [], [], []) is not None              # no line: nothing to do
    good = 1 << 2
    # a Good line whose distances match none of the three cases
    call_candidates(engine, [0, 1, 2], [0, good, 0], [20, 50, 20], [20, 8, 20], expect_error="line 1 is Good")
    call_candidates(engine, [0, 1, 2], [0, good | 3, 0], [20, 20, 20], [20, 20, 20], expect_error="line 1 is Good")   # both `None`
    # a neighbour before the first line, behind the last one
    call_candidates(engine, [0, 1], [good, 0], [20, 0], [0, 0], expect_error="line 0 is Good")
    call_candidates(engine, [0, 1], [0, good], [0, 0], [0, 20], expect_error="line 1 is Good")
    call_candidates(engine, [0, 5], [0, 0], [0, 0], [0, 0], expect_error="names no group")


# ------------------------------------------------------------------------------------------------------------ prune
def test_prune_reproduces_every_case(engine):
    records, mirnas, cand_mir = case_arrays(CASES)
    got = call_prune(engine, np.arange(len(CASES)), cand_mir, records, mirnas)
    n_host = 0
    for c, (seq, structure, mirs, pruned, _) in enumerate(CASES):
        status, lo, hi = cases.prune_expected(seq, structure, mirs)
        assert (got["status"][c], got["lo"][c], got["hi"][c]) == (status, lo, hi), (c, seq, structure, mirs)
        text = got["pruned"][int(got["off"][c]):int(got["off"][c + 1])].decode()
        if status == 2:
            n_host += 1
            assert len(seq) == 257 and text == ""
        else:
            assert text == (pruned or ""), (c, seq, structure, mirs)       # the reference's own slice
    assert n_host == 8 and int(got["off"][-1]) == len(got["pruned"])


@pytest.mark.parametrize("n", [0, 1, WAVES - 1, WAVES, WAVES + 1])
def test_prune_candidate_counts_around_a_workgroup(engine, n):
    which = [c for c in CASES if c[3] and len(c[0]) > 60][:5]
    records, mirnas, cand_mir = case_arrays(which)
    pick = [4, 2, 0, 3, 1][:n]
    got = call_prune(engine, pick, cand_mir[pick] if n else np.zeros((0, 2), np.uint32), records, mirnas)
    assert got["pruned"].decode() == "".join(which[k][3] for k in pick) and got["status"].tolist() == [1] * n


def test_prune_skips_unused_slots_and_takes_the_second_mirna(engine):
    seq = "A" * 20 + "GGGGCCAUAGGCCCC" + "A" * 25
    structure = "." * 20 + "((((.......))))" + "." * 25
    records, mirnas = [(seq, structure)], ["GGGGCC", "CAUAG", "AAAAAAAAAAAAAAAAAAAAG"]
    got = call_prune(engine, [0, NO, 0, 0], [[0, NO], [NO, NO], [0, 1], [2, 1]], records, mirnas)
    want = [model.prune_slice(seq, structure, m) for m in (["GGGGCC"], ["GGGGCC", "CAUAG"], ["AAAAAAAAAAAAAAAAAAAAG", "CAUAG"])]
    # the first miRNA stands at 20: it is the one; otherwise the second, which lies in the loop: no `)` before its end
    assert want[0] == want[1] == seq[5:50] and want[2] is None
    assert got["status"].tolist() == [1, 3, 1, 0] and got["pruned"].decode() == want[0] * 2
    assert got["lo"].tolist() == [5, 0, 5, 0] and got["hi"].tolist() == [50, 0, 50, 0]


def test_prune_refuses_contradicting_arrays(engine):
    records, mirnas = [("ACGUACGU", "((....))"), ("ACGU", "....")], ["ACG"]
    ok = call_prune(engine, [0, 1], [[0, NO], [0, NO]], records, mirnas)
    assert ok["status"].tolist() == [1, 0]
    call_prune(engine, [0, 1], [[0, NO], [0, NO]], records, mirnas, rec_off=[0, 8, 11], expect_error="offsets")      # do not close
    call_prune(engine, [0, 1], [[0, NO], [0, NO]], records, mirnas, rec_off=[0, 13, 12], expect_error="offsets")     # do not ascend
    call_prune(engine, [0, 1], [[0, NO], [0, NO]], records, mirnas, rec_off=[4, 2, 12], expect_error="offsets")
    call_prune(engine, [0, 2], [[0, NO], [0, NO]], records, mirnas, expect_error="no record or no miRNA")
    call_prune(engine, [0, 1], [[0, NO], [1, NO]], records, mirnas, expect_error="no record or no miRNA")
    call_prune(engine, [0, 1], [[0, 7], [0, NO]], records, mirnas, expect_error="no record or no miRNA")
    call_prune(engine, [0, 1], [[0, NO], [0, NO]], [("ACGUACGU", "((....)."), ("ACGU", "....")], mirnas, expect_error="candidate 0")
    call_prune(engine, [1, 0], [[0, NO], [0, NO]], [("ACGUACGU", ".(....))"), ("ACGU", "....")], mirnas, expect_error="candidate 1")
    call_prune(engine, [0], [[0, NO]], [("ACG", "...")], ["UUUUU"], expect_error="candidate 0")      # the reference's IndexError
    call_prune(engine, [0, 1], [[0, NO], [0, NO]], records, mirnas, cap=7, expect_error="room for 7")


# --------------------------------------------------------------------------------------------------------- features
def test_features_reproduce_every_case_and_leave_exactly_the_built_ones_to_the_host(engine):
    records, mirnas, cand_mir = case_arrays(CASES)
    got = call_features(engine, np.ones(len(CASES), np.uint8), cand_mir, records, mirnas)
    host_cases = 0
    for c, (seq, structure, mirs, _, feat) in enumerate(CASES):
        want = cases.row_of(seq, structure, mirs)
        assert got[c, 0] == want[0], (c, seq, structure, mirs)
        if want[0] == 2:
            host_cases += 1
            assert cases.takes_host_path(seq, structure)
            continue
        assert got[c].tolist() == want, (c, seq, structure, mirs, dict(zip(cases.WORDS, got[c].tolist())))
        assert (feat is None) == (want[0] == 0)
        if feat is not None:      # the reference's own numbers
            arms = {cases.ARMS[got[c, 4]]: [int(got[c, 6]), int(got[c, 7])]}
            if got[c, 8] >= 0:
                arms[cases.ARMS[got[c, 8]]] = [int(got[c, 9]), int(got[c, 10])]
            assert [got[c, 1], got[c, 2], got[c, 3], cases.ARMS[got[c, 4]], got[c, 5], arms, got[c, 11], "Yes" if got[c, 12] else "No"] == feat[:8]
            assert (got[c, 13] / float(got[c, 14]) if got[c, 14] else 0) == feat[10] and got[c, 13] == feat[11]
    assert host_cases == HOST_CASES


@pytest.mark.parametrize("n", [0, 1, WAVES - 1, WAVES, WAVES + 1])
def test_features_candidate_counts_around_a_workgroup(engine, n):
    which = [c for c in CASES if c[4] is not None and 60 < len(c[0]) <= 256 and not cases.takes_host_path(c[0], c[1])][:5]
    pick = [4, 2, 0, 3, 1][:n]
    records, mirnas, cand_mir = case_arrays([which[k] for k in pick])
    status = np.ones(n, np.uint8)
    if n > 1:
        status[1] = 0             # (a candidate that was not cut: the all-None row, whatever its strings hold)
    got = call_features(engine, status, cand_mir, records, mirnas)
    for c, k in enumerate(pick):
        want = cases.row_of(*which[k][:3]) if status[c] else [0] * 8 + [-1] + [0] * 7
        assert got[c].tolist() == want


def test_features_refuse_contradicting_arrays_and_structures_rnafold_does_not_write(engine):
    pruned, mirnas = [("ACGUACGU", "((....))"), ("ACGUAC", "(....)")], ["ACG"]
    mir = [[0, NO], [0, NO]]
    assert call_features(engine, [1, 1], mir, pruned, mirnas)[:, 0].tolist() == [1, 1]
    call_features(engine, [1, 1], mir, pruned, mirnas, p_off=[0, 8, 13], expect_error="offsets")
    call_features(engine, [1, 1], mir, pruned, mirnas, p_off=[0, 15, 14], expect_error="offsets")
    call_features(engine, [1, 1], mir, pruned, mirnas, p_off=[1, 8, 14], expect_error="offsets")
    call_features(engine, [1, 1], [[0, NO], [3, NO]], pruned, mirnas, expect_error="no miRNA")
    assert call_features(engine, [1, 0], [[0, NO], [3, NO]], pruned, mirnas)[:, 0].tolist() == [1, 0]      # (not looked at)
    call_features(engine, [1, 1], mir, [pruned[0], ("ACGUAC", "((..))")], mirnas, expect_error="record 1")   # a hairpin loop of 2
    call_features(engine, [1, 1], mir, [("ACGUACGU", "((....)."), pruned[1]], mirnas, expect_error="record 0")
    call_features(engine, [1, 1], mir, [pruned[0], ("ACGUAC", ")....(")], mirnas, expect_error="record 1")


# ----------------------------------------------------------------------------------------------------------- select
@pytest.mark.parametrize("w", WORLDS, ids=lambda w: w["name"])
def test_select_of_the_worlds(engine, w):
    a = cases.world_arrays(w)
    best = call_select(engine, a["cand_n"], a["cand_rec"], a["rec_mfe"], a["feat"])
    assert best.tolist() == a["best"].tolist()


def test_select_prefers_the_retained_then_the_lowest_energy_then_the_lower_slot(engine):
    def row(bindings=20, arm=1, over=0, hairpins=1, bound=20, mir_len=22, state=1):
        return [state, hairpins, bindings, 0, arm, 5, over, 3, -1, 0, 0, bindings, 0, bound, mir_len, 1]
    null = [0] * 8 + [-1] + [0] * 7
    lines = [
        ([row(), row(), null, null], [-5.0, -5.0], 0),                      # a tie: the lower slot
        ([row(), row(), null, null], [-5.0, -6.0], 1),                      # the lower energy
        ([row(bindings=14), row(), null, null], [-9.0, -1.0], 1),           # the retained one before the lower energy
        ([row(bindings=14), row(over=6), null, null], [-1.0, -9.0], 1),     # none retained: all of them, the lower energy
        ([null, null, null, null], [-1.0, -2.0], -1),                       # all null
        ([null, row(arm=2, over=1), null, null], [-1.0, -2.0], 1),          # arm3 with an overlap: not retained, but the only one
        ([row(bound=13), row(bound=14, mir_len=23), null, null], [-9.0, -1.0], 1),   # 13/22 < 0.6 <= 14/23
        ([row(arm=0), row(arm=3), row(arm=2), row(arm=2, over=1)], [-9.0, -8.0, -1.0, -7.0], 2),   # four: loop, unmatched, arm3
    ]
    n = len(lines)
    cand_n = np.array([2] * (n - 1) + [4], np.uint8)
    cand_rec = np.full(4 * n, NO, np.uint32)
    rec_mfe = np.zeros(2 * n)
    feat = np.zeros((4 * n, 16), np.int32)
    for i, (rows, mfes, _) in enumerate(lines):
        feat[4 * i:4 * i + 4] = rows
        if len(mfes) == 2:
            cand_rec[4 * i:4 * i + 2] = [2 * i, 2 * i + 1]
            rec_mfe[2 * i:2 * i + 2] = mfes
        else:   # four candidates: the neighbours' records carry the outer energies
            cand_rec[4 * i:4 * i + 4] = [2 * i - 1, 2 * i, 2 * i + 1, 2 * i - 2]
            rec_mfe[[2 * i - 1, 2 * i, 2 * i + 1, 2 * i - 2]] = mfes
    best = call_select(engine, cand_n, cand_rec, rec_mfe, feat)
    assert best.tolist() == [x[2] for x in lines]
    left = feat.copy()
    left[1, 0] = 2
    call_select(engine, cand_n, cand_rec, rec_mfe, left, expect_error="left to the host")
    call_select(engine, cand_n, cand_rec, rec_mfe, feat, n_rec=2 * n - 1, expect_error="every line has two")
    three = cand_n.copy()
    three[0] = 3
    call_select(engine, three, cand_rec, rec_mfe, feat, expect_error="neither two nor four")


# ------------------------------------------------------------------------------------------------------- end to end
def counted_fold(tmp_path):
    """A wrapper around the stand-in that appends a line to a log every time it is started: (path, log path)."""
    log, path = str(tmp_path / "fold_calls.log"), str(tmp_path / "counted_fold.sh")
    with open(path, "w") as fh:
        fh.write("#!/bin/sh\necho \"$@\" >> '%s'\nexec '%s' '%s' \"$@\"\n" % (log, sys.executable, cases.STANDIN))
    os.chmod(path, os.stat(path).st_mode | stat.S_IXUSR)
    return path, log


@pytest.mark.parametrize("w", WORLDS, ids=lambda w: w["name"])
def test_worlds_end_to_end_equal_the_reference(engine, tmp_path, w):
    from mirge_amd import predict
    a = cases.world_arrays(w)
    n = a["n"]
    stem = str(tmp_path / "unmapped_mirna_smp")
    for suffix, text in (("_features.tsv", w["features"]), ("_features_precusor.fa", w["precursors"])):
        with open(stem + SUFFIX + suffix, "w") as fh:
            fh.write(text)
    up, down = np.array(a["up"], np.int64).reshape(-1), np.array(a["down"], np.int64).reshape(-1)
    feats = dict(nb_flags=flags_of(a["states"], a["up"], a["down"]), nb_up=up, nb_down=down)
    prec = dict(rec_group=np.repeat(np.arange(n, dtype=np.uint32), 2), records=2 * n)
    cmd, log = counted_fold(tmp_path)
    timings = {}
    got = predict.screen_precursors(engine, feats, prec, cmd, stem, timings=timings)
    assert open(stem + SUFFIX + "_features_updated_stableClusterSeq_15.tsv").read() == w["table"]
    assert got["lines"] == n and got["host_candidates"] == 0 and got["best"].tolist() == a["best"].tolist()
    assert got["candidates"] == int(a["cand_n"].sum()) and got["pruned"] == int((np.diff(a["p_off"].astype(np.int64)) > 0).sum())
    if n:
        assert open(log).read() == "--noPS --noLP\n" * 2 and got["folds"] == 2          # twice a sample, not once a candidate
        assert open(stem + SUFFIX + "_features_precusor.str").read() == w["str"]
        assert set(timings) >= {"fold1_s", "fold2_s", "parse_s", "device_s", "host_s", "write_s", "host_candidates"}
    else:
        assert not os.path.exists(log) and got["folds"] == 0


def host_world():
    """Three lines that are not Good: two whose records are beyond 256 characters, and one whose miRNA closes a multiloop of
    ten hairpins, so that its pruned structure has eleven stems.  (features text, FASTA text)."""
    rng = np.random.default_rng(5)
    dna = lambda k: "".join("ACGT"[c] for c in rng.integers(0, 4, k))
    rc = lambda s: s.translate(str.maketrans("ACGT", "TGCA"))[::-1]
    arm, outer = dna(22), dna(22)
    long_rec = dna(150) + arm + dna(8) + rc(arm) + dna(80)
    units = "".join(x + "AAAAA" + rc(x) + "AA" for x in ("GGGC", "GCGG", "CGGG", "GGCC", "CCGG", "GCCG", "CGCG", "GGGG", "CCCC", "GCGC"))
    many = "A" * 16 + outer + "AA" + units + rc(outer) + "A" * 16
    mirnas = [arm, arm, outer]
    header = "\t".join(["x"] * 5 + ["clusterName", "clusterSeq", "majoritySeq", "stableClusterSeq", "neighborState", "upstreamDistance",
                                      "downstreamDistance"]) + "\n"
    features = header + "".join("\t".join(["."] * 5 + ["smp:c%d" % i, ".", ".", m, "Null", "None", "None"]) + "\n" for i, m in enumerate(mirnas))
    records = [long_rec, long_rec[10:], long_rec[:200], long_rec, many, many[4:]]
    fasta = "".join(">smp:c%d:precusor_%d\n%s\n" % (k // 2, 1 + k % 2, s.replace("T", "U")) for k, s in enumerate(records))
    return features, fasta


def host_candidates_of(features, str_text):
    """The candidates the kernels must leave to the host, by the model: (count, of them beyond 256 characters, many-stemmed)."""
    records = model.parse_str(str_text)
    _, lines = model.screen_lines(features, str_text, cases.fold_many)
    long_ones = many = both = 0
    for d in lines:
        for r, (p, structure, f) in zip(d["records"], d["candidates"]):
            is_long = len(records[r][1]) > 256
            is_many = f is not None and (f["n_stems"] >= 10 or f["hairpin_count"] >= 10)
            long_ones, many, both = long_ones + is_long, many + is_many, both + (is_long and is_many)
    return long_ones + many - both, long_ones, many


def test_screen_precursors_works_long_and_many_stemmed_candidates_out_on_the_host(engine, tmp_path):
    from mirge_amd import predict
    features, fasta = host_world()
    stem = str(tmp_path / "unmapped_mirna_smp")
    for suffix, text in (("_features.tsv", features), ("_features_precusor.fa", fasta)):
        with open(stem + SUFFIX + suffix, "w") as fh:
            fh.write(text)
    feats = dict(nb_flags=np.full(3, 3, np.uint8), nb_up=np.zeros(3, np.int64), nb_down=np.zeros(3, np.int64))
    got = predict.screen_precursors(engine, feats, dict(rec_group=np.repeat(np.arange(3, dtype=np.uint32), 2), records=6), cases.fold_file, stem)
    str_text = open(stem + SUFFIX + "_features_precusor.str").read()
    count, long_ones, many = host_candidates_of(features, str_text)
    assert long_ones == 3 and many >= 1
    assert open(got["path"]).read() == model.screen(features, str_text, cases.fold_many)
    assert got["host_candidates"] == count and got["lines"] == 3 and got["folds"] == 2


def test_map_and_cluster_with_screen_equals_the_model(engine, oracle_lib, tmp_path):
    from mirge_amd import predict
    from mirge_amd.index import FmIndex
    from tests.test_gpu_predict_precursors import synthetic_genome
    from tests.test_gpu_predict_trim import REPEATS_TSV
    names, texts, reads = synthetic_genome(np.random.default_rng(48))
    genome_prefix = str(tmp_path / "syn_genome")
    FmIndex.build(names, texts).save(genome_prefix + ".mrgfm")
    reads = list(dict.fromkeys(reads))
    fa = tmp_path / "unmapped_mirna_s1.fa"
    fa.write_text("".join(">mir%d_%d\n%s\n" % (k + 5, 2 + k % 5, r) for k, r in enumerate(reads)))
    (tmp_path / "rep.tsv").write_text(REPEATS_TSV)
    prec, screen, shell = tmp_path / "prec", tmp_path / "screen", tmp_path / "shell"
    for d in (prec, screen, shell):
        d.mkdir()
    base = "unmapped_mirna_s1"
    trim = (str(tmp_path / "rep.tsv"), 24)
    cmd, log = counted_fold(tmp_path)
    args = dict(trim=trim, remap=True, features=True, precursors=True)
    cl0 = predict.map_and_cluster(engine, str(fa), genome_prefix, 3, 25, 14, str(prec / base), **args)
    cl = predict.map_and_cluster(engine, str(fa), genome_prefix, 3, 25, 14, str(screen / base), screen=True, fold=cmd, **args)
    table = base + SUFFIX
    new = [table + s for s in ("_features_precusor_tmp.str", "_features_precusor.str", "_features_pruned_15.fa", "_features_pruned_15.str",
                               "_features_updated_stableClusterSeq_15.tsv")]
    old = sorted(os.listdir(str(prec)))
    assert sorted(os.listdir(str(screen))) == sorted(old + new)
    for fn in old:
        assert (prec / fn).read_bytes() == (screen / fn).read_bytes(), fn
    assert sorted(set(cl) - set(cl0)) == ["screen"]
    want = model.screen((screen / (table + "_features.tsv")).read_text(), (screen / new[1]).read_text(), cases.fold_many)
    assert (screen / new[4]).read_text() == want
    assert cl["screen"]["lines"] == cl["features"]["lines"] > 6 and cl["screen"]["folds"] == 2
    assert open(log).read() == "--noPS --noLP\n" * 2
    with pytest.raises(ValueError, match="screen needs fold"):
        predict.map_and_cluster(engine, str(fa), genome_prefix, 3, 25, 14, str(screen / "x"), screen=True, **args)
    os.remove(log)
    assert predict.main(["clusters", genome_prefix, str(fa), "-o", str(shell / base), "--trim", "--repeats", str(tmp_path / "rep.tsv"),
                         "-clc", "24", "--remap", "--features", "--precursors", "--screen", "--fold-cmd", cmd]) == 0
    assert sorted(os.listdir(str(shell))) == sorted(os.listdir(str(screen)))
    assert (shell / new[4]).read_bytes() == (screen / new[4]).read_bytes()
    assert open(log).read() == "--noPS --noLP\n" * 2


def test_cli_novel_screen_adds_the_table_per_sample(tmp_path_factory, native_lib, oracle_lib, tmp_path):
    from mirge_amd import cli
    from mirge_amd.index import FmIndex
    from tests import util
    from tests.test_gpu_predict_precursors import synthetic_genome
    from tests.test_gpu_predict_trim import REPEATS_TSV
    w = util.World(n_fixed=600, n_var=150)
    root = str(tmp_path_factory.mktemp("screen_libs") / "libs")
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
    cmd, log = counted_fold(tmp_path)
    res = cli.annotate_main(cli.build_parser().parse_args(
        ["annotate", "-s"] + fastqs + ["-lib", root, "-sp", "syn", "-o", str(tmp_path / "screen"), "--novel-screen", "--fold-cmd", cmd,
                                       "-pr", "/nowhere", "-clc", "24", "-sl", "18"]))
    out = os.path.join(res["outdir"], "unmapped_tmp")
    for stem in ("left", "right"):
        sub = os.path.join(out, "unmapped_mirna_%s_tmp" % stem)
        table = "unmapped_mirna_" + stem + SUFFIX
        assert {table + ".tsv", table + "_features.tsv", table + "_features_precusor.fa", table + "_features_precusor.str",
                table + "_features_updated_stableClusterSeq_15.tsv"} <= set(os.listdir(sub))
        features = open(os.path.join(sub, table + "_features.tsv")).read()
        want = model.screen(features, open(os.path.join(sub, table + "_features_precusor.str")).read(), cases.fold_many)
        assert open(os.path.join(sub, table + "_features_updated_stableClusterSeq_15.tsv")).read() == want
        assert want.count("\n") == features.count("\n") > 1
    assert open(log).read() == "--noPS --noLP\n" * 4          # twice a sample
