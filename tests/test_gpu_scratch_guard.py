"""Every stage that takes caller scratch stays inside the bytes its mrg_*_temp_bytes call reports.  For the length of a
test Engine._tmp (the one place where stage scratch is allocated) is replaced by a wrapper that allocates GUARD bytes
more than the sizing call asks for, fills all of it with 0xA5 and hands the stage the first `need` bytes, so that the
library is told exactly `need`.  A stage runs once as it is and once over the wrapper: the guards must still hold 0xA5 and
the results must be equal.  An overrun lands inside the same allocation: the test can fail, it cannot fault.

The inputs are the hand-made worlds of the stages' own tests (tens of rows).  A touched guard is a finding about a layout of
capi.hip (the Carver's pieces and the kernels' extents disagree): mend the layout, not the guard."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from tests import predict_features_cases as feature_cases
from tests import predict_precursors_cases as precursor_cases
from tests import predict_remap_model as remap_model
from tests import predict_screen_cases as screen_cases
from tests import predict_screen_model as screen_model
from tests import predict_trim_model as trim_model

pytestmark = pytest.mark.gpu

GUARD, FILL = 4096, 0xA5
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NO = screen_cases.NO


@pytest.fixture(scope="module")
def engine(native_lib):
    from mirge_amd.engine import Engine
    eng = Engine(0)
    yield eng
    eng.close()


def world(fixture, name):
    with open(os.path.join(GOLDEN, fixture)) as fh:
        return next(w for w in json.load(fh)["worlds"] if w["name"] == name)


class Guarded:
    """The stand-in for Engine._tmp: keeps every full buffer and where its guard begins."""

    def __init__(self, engine):
        self.engine, self.buffers = engine, []

    def __call__(self, sizer, *sizes, floor=0):
        import torch
        from mirge_amd._native import check
        need = C.c_uint64()
        check(sizer(*[int(s) for s in sizes], C.byref(need)))
        need = int(need.value)      # (the stage's floor is left out: the library is told what its own sizing call said)
        full = torch.full((need + GUARD,), FILL, dtype=torch.uint8, device=self.engine.device)
        self.buffers.append((full, need))
        return full[:need]

    def guards_intact(self):
        for full, need in self.buffers:
            tail = full[need:].cpu().numpy()
            assert tail.shape[0] == GUARD and (tail == FILL).all(), "a stage wrote %d bytes past its %d of scratch" % (
                int(np.flatnonzero(tail != FILL)[-1]) + 1, need)
        return True


def plain(x):
    """A stage's result as host values that compare with ==; what a stage keeps on the device for the next one ("device")
    is left out: its buffers are longer than what the stage fills."""
    import torch
    if isinstance(x, dict):
        return {k: plain(v) for k, v in x.items() if k != "device"}
    if isinstance(x, (list, tuple)):
        return [plain(v) for v in x]
    if torch.is_tensor(x):
        x = x.cpu().numpy()
    if isinstance(x, np.ndarray):
        return (str(x.dtype), x.shape, x.tobytes())
    return x


def check_stage(engine, monkeypatch, run, min_buffers=1):
    """run(engine) as it is and over the guarded scratch: equal results, untouched guards, and the wrapper was what ran."""
    want = plain(run(engine))
    guarded = Guarded(engine)
    monkeypatch.setattr(engine, "_tmp", guarded)
    got = plain(run(engine))
    monkeypatch.undo()
    assert len(guarded.buffers) >= min_buffers, "the stage did not take its scratch from Engine._tmp"
    assert guarded.guards_intact()
    assert got == want
    return got


def hand_reads():
    from mirge_amd import pack
    rng = np.random.default_rng(7)
    seqs = ["".join("ACGT"[c] for c in rng.integers(0, 4, int(L))) for L in rng.integers(16, 40, 37)]
    seqs[5] = seqs[4]                         # equal strings, a prefix of another, an N
    seqs[9] = seqs[8][:17]
    seqs[11] = seqs[11][:6] + "N" + seqs[11][7:]
    quant = rng.integers(0, 4, (len(seqs), 3)).astype(np.uint32)
    quant[:, 2] = 0                           # a sample without reads
    return pack.pack_reads(seqs), quant


def test_seq_rank_and_collapsed_order(engine, monkeypatch):
    (words, lens, nmask), quant = hand_reads()
    got = check_stage(engine, monkeypatch, lambda e: e.collapsed_order(words, lens, nmask, quant), min_buffers=2)
    assert [len(o[2]) // 4 for o in got] == [int((quant[:, s] > 0).sum()) for s in range(3)]


def test_predict_select_sample_reads_and_gather(engine, monkeypatch):
    (words, lens, nmask), quant = hand_reads()
    pass_id = np.where(np.arange(len(lens)) % 3 == 0, 0, -1).astype(np.int8)

    def run(e):
        sel = e.predict_select(pass_id, lens, quant, 16, 30, 2)
        rows = [e.predict_sample_reads(quant, sel[key], s, thr) for s in range(3) for key, thr in (("raw_no", 1), ("sel_no", 2))]
        picked = [e.predict_gather(words, lens, nmask, quant, r[0], sample=s) for r, s in ((rows[0], 0), (rows[3], 1), (rows[1], None))]
        return sel, rows, picked
    sel = check_stage(engine, monkeypatch, run, min_buffers=10)[0]
    assert sel["n_raw"] >= sel["n_sel"] > 0


def test_predict_trim(engine, monkeypatch, tmp_path):
    from mirge_amd import predict
    from mirge_amd.index import FmIndex
    w = world("predict_trim.json", "two_elements")
    entries, rows, a, *_, rep_tsv = trim_model.world_inputs(w["table"], w["elements"])
    (tmp_path / "rep.tsv").write_text(rep_tsv)
    repeats = predict.load_repeats(str(tmp_path / "rep.tsv"), [FmIndex.build(list(entries), ["ACGTTGCAAC" * 3] * len(entries))])
    cl = dict(a, seq=a["seq"].encode())
    got = check_stage(engine, monkeypatch, lambda e: e.predict_trim(cl, repeats, w["cutoff"]))
    assert got["flag"][1] == (len(rows),) and len(got["kept"][2]) // 4 == w["trimmed_fa"].count(">")


def test_predict_trim_reads_and_remap_rows(engine, monkeypatch, tmp_path):
    from mirge_amd import pack, predict
    from mirge_amd.engine import ReadSet
    from mirge_amd.index import FmIndex
    w = world("predict_remap.json", "sl18")
    names, seqs = remap_model.parse_fasta(w["reads_fa"])
    kept = remap_model.cluster_arrays(w["clusters_fa"])[2]
    stem = str(tmp_path / "unmapped_mirna_smp")
    with open(stem + "_vs_genome_sorted_clusters_trimmed_orig.fa", "w") as fh:
        fh.write(w["clusters_fa"])
    rs = ReadSet(*pack.pack_reads(seqs), device=engine.device)
    numbers = np.array([remap_model.read_number(n) for n in names], np.uint32)
    # (predict.map_reads_to_clusters does this on an engine of its own: here the clusters join the test's engine)
    index = FmIndex.from_fasta(stem + "_vs_genome_sorted_clusters_trimmed_orig.fa", device=engine.device_index)
    engine.add_library("guard_clusters", index, exact_dict=False)
    run = lambda e: e.predict_remap(rs, numbers, "guard_clusters", np.array(kept, np.uint32), w["seed_length"], predict.REMAP_TRIMS)
    got = check_stage(engine, monkeypatch, run, min_buffers=2)       # (the cut reads' scratch and the rows')
    assert got["n_rows"] == len(w["table"].splitlines()) > 0


def feature_world(engine):
    from tests.test_gpu_predict_features import world_inputs
    t = feature_cases.golden_worlds()[1]                             # "mapped": two chromosomes, a handful of rows
    a = feature_cases.Arrays(t["table"], t["chromosomes"])
    rs, parts, trim, remap = world_inputs(engine, a)
    cl = dict(a.cl, kept=a.kept, kept_seq_off=a.kept_seq_off, kept_orig=a.kept_orig)
    return a, rs, remap, cl


def test_predict_features(engine, monkeypatch):
    a, rs, remap, cl = feature_world(engine)
    run = lambda e: e.predict_features(rs, a.counts, remap["device"], cl, a.entry_len, a.entry_rank, lambda g, lo, hi, c: None)
    got = check_stage(engine, monkeypatch, run)
    assert got["n_groups"] > 0 and got["n_sorted"] > 0


def test_predict_precursors(engine, monkeypatch):
    from tests.test_gpu_predict_precursors import Dev, resident
    w = next(w for w in precursor_cases.golden()["worlds"] if w["name"] == "hand")
    a = precursor_cases.Arrays(w["features"], w["chromosomes"])
    parts, _ = a.indexes()
    keys = resident(engine, parts, "guard_" + w["name"])
    d = Dev(engine)
    dev = dict(order=d.up(a.order, np.uint32), group_cluster=d.up(a.group_cluster, np.uint32), frame=d.up(a.frame, np.int32),
               valid=d.up(a.valid, np.uint8), n_sorted=a.n_groups, n_groups=a.n_groups)
    got = check_stage(engine, monkeypatch, lambda e: e.predict_precursors(dev, a.cl, a.entry_len, keys))
    assert got["n_written"] == a.n_groups > 0 and got["seq"] == a.rec["seq"]


def test_predict_screen_calls(engine, monkeypatch):
    from tests.test_gpu_predict_screen import flags_of
    w = next(w for w in screen_cases.golden()["worlds"] if w["name"] == "screen_hand")
    _, rows = screen_model.read_features(w["features"])
    records = screen_model.parse_str(w["str"])
    n = len(rows)
    states, up, down = [r[3] for r in rows], np.array([r[4] for r in rows], np.int64), np.array([r[5] for r in rows], np.int64)
    rec_off, rec_seq = screen_cases.blob([r[1] for r in records])
    rec_str = screen_cases.blob([r[2] for r in records])[1]
    mir_off, mir = screen_cases.blob([r[2] for r in rows])
    # the two later calls on hand-made rows (the worlds' need a fold between the calls): two cut candidates, one line of two
    p_off, p_seq = screen_cases.blob(["ACGUACGU", "ACGUAC"])
    p_str = screen_cases.blob(["((....))", "(....)"])[1]
    m_off, m = screen_cases.blob(["ACG"])
    feat_row = [1, 1, 20, 0, 1, 5, 0, 3, -1, 0, 0, 20, 0, 20, 22, 1]
    feat = np.array([feat_row, feat_row, [0] * 8 + [-1] + [0] * 7, [0] * 8 + [-1] + [0] * 7], np.int32)

    def run(e):
        cands = e.predict_screen_candidates(np.arange(n, dtype=np.uint32), flags_of(states, up, down), up, down)
        pruned = e.predict_screen_prune(cands["cand_rec"], cands["cand_mir"], rec_off, rec_seq, rec_str, mir_off, mir)
        words = e.predict_screen_features(np.ones(2, np.uint8), np.array([0, NO, 0, NO], np.uint32), p_off, p_seq, p_str, m_off, m)
        best = e.predict_screen_select(np.array([2], np.uint8), np.array([0, 1, NO, NO], np.uint32), np.array([-1.0, -2.0]), feat)
        return cands, pruned, words, best
    cands, pruned, words, best = check_stage(engine, monkeypatch, run, min_buffers=4)
    assert n > 0 and len(pruned["pruned"]) > 0 and best[1] == (1,)
