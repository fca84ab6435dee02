"""Tied ungapped alignments of `-ai` on the GPU: mrg_a2i_settle (csrc/a2i_align.hip) against its model
(tests/a2i_settle_model.py) field by field, which rows stay status 1 included, and `annotate -ai` on a tie-heavy world
against `--ai-host`."""
import ctypes as C
import itertools
import json
import os
import random

import numpy as np
import pytest

from mirge_amd import a2i, pack
from tests import a2i_align_model as model
from tests import a2i_settle_model as settle
from tests.conftest import ROOT
from tests.test_gpu_a2i_align import assert_same, golden_layout, run_ai, world_of

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng(native_lib):
    from mirge_amd.engine import Engine
    return Engine(0)


def status_of(rec):
    return rec[:, 0] & 0xFF


def run_pairs(eng, pairs, W=None, **kw):
    """Engine.a2i_align with and without settle against the two models -> (rec settled, examined, settled)."""
    table, seqs, pass_id, ref_id = world_of(pairs)
    words, lens, nmask = pack.pack_reads(seqs, W)
    idx0, rec0 = eng.a2i_align(table, words, lens, nmask, pass_id, ref_id, **kw)
    timings = {}
    idx, rec = eng.a2i_align(table, words, lens, nmask, pass_id, ref_id, settle=True, timings=timings, **kw)
    w_idx, w_rec0 = model.records(table, seqs, pass_id, ref_id, **kw)
    w_rec, examined, settled = settle.settle_records(table, seqs, w_idx, w_rec0, **kw)
    assert np.array_equal(idx0, w_idx) and np.array_equal(idx, w_idx)
    assert_same(rec0, w_rec0, pairs)                                   # settle=False: as before
    assert_same(rec, w_rec, pairs)
    other = status_of(rec0) != model.ENDS
    assert np.array_equal(rec[other], rec0[other])                     # rows of status 0, 2, 3 and 4: byte for byte
    assert (timings["settle_examined"], timings["settle_settled"]) == (examined, settled)
    assert examined == 0 or timings["settle_kernel_ms"] > 0
    return rec, examined, settled


@pytest.mark.parametrize("world", ["ties", "random", "random99", "isomir"])
def test_kernel_equals_the_model_on_the_worlds(eng, world):
    pairs = {"ties": lambda: model.TIE_CASES + [(t, s) for t, s, _ in settle.COUNTEREXAMPLES],
             "random": lambda: model.random_pairs(2000), "random99": lambda: model.random_pairs(2000, seed=99),
             "isomir": lambda: model.isomir_world(600, 20, 7)[:2000]}[world]()
    rec, examined, settled = run_pairs(eng, pairs)
    assert 0 < settled <= examined
    if world == "ties":
        assert rec[-3:, 1].tolist() == [d for _, _, d in settle.COUNTEREXAMPLES]
    if world.startswith("random"):
        assert settled > 400 and (status_of(rec) == model.ENDS).any() and (status_of(rec) == model.GAPPED).any()


def test_every_length_pair_over_one_and_two_letters(eng):
    """Ties on every diagonal, and in the last row and the last column, whose cells pairwise2 lists as best cells too."""
    rnd = random.Random(17)
    pairs = []
    for la, lb in itertools.product((1, 5, 6, 31, 32), repeat=2):
        pairs.append(("A" * la, "A" * lb))
        for _ in range(8):
            pairs.append(("".join(rnd.choice("AC") for _ in range(la)), "".join(rnd.choice("AC") for _ in range(lb))))
        for _ in range(3):
            pairs.append(("".join(rnd.choice("AAC") for _ in range(la)), "".join(rnd.choice("AAAC") for _ in range(lb))))
    rec, examined, settled = run_pairs(eng, pairs)
    assert len(pairs) == 300 and settled > 150
    tied = rec[status_of(rec) == settle.TIED]
    assert tied[:, 1].min() <= -20 and tied[:, 1].max() >= 20 and ((tied[:, 0] >> 8) & 1).any() and ((tied[:, 0] >> 9) & 1).any()


def test_n_in_the_read_other_bases_and_two_words(eng):
    rnd = random.Random(23)
    with_n = []
    for t, s in model.random_pairs(400, seed=3):
        s = list(s)
        s[rnd.randrange(len(s))] = "N"
        with_n.append((t, "".join(s)))
    with_n += [("A" * 20, "AAAANAAAAAAAAANAAAA"), ("AC" * 11, "ACACACNCACACACACAC"), ("A" * 32, "N" + "A" * 31), ("A" * 32, "A" * 31 + "N")]
    _, _, settled = run_pairs(eng, with_n)
    assert settled > 40
    ct = []
    for _ in range(300):
        alpha = rnd.choice(["CT", "CCT", "ACT"])
        t = "".join(rnd.choice(alpha.replace("T", "C") + "C") for _ in range(rnd.randint(16, 27)))
        ct.append((t, "".join(rnd.choice(alpha) for _ in range(rnd.randint(14, 24)))))
        ct.append((t, t[rnd.randint(0, 3):len(t) - rnd.randint(0, 3)].replace("C", "T", 1)))
    rec, _, settled = run_pairs(eng, ct, from_base="C", to_base="T")
    assert settled > 40 and (rec[status_of(rec) == settle.TIED][:, 2] != 0).any()
    rec, _, settled = run_pairs(eng, model.random_pairs(300, seed=8) + [("ACGT" * 5, "ACGT" * 9)], W=2)
    assert settled > 40 and status_of(rec)[-1] == model.UNSUPPORTED


# ------------------------------------------------------------------ the entry point itself, on rows uploaded from the model
@pytest.fixture(scope="module")
def pool():
    """~400 distinct pairs of every status, their records before and after settling (the model's), computed once."""
    pairs = model.random_pairs(380, seed=41) + [("A" * 20, "C" * 20), ("ACGT" * 5, "ACGT" * 9), ("AC" * 11, "N" * 12)]
    pairs = list(dict.fromkeys(pairs))
    table, seqs, pass_id, ref_id = world_of(pairs)
    idx, rec1 = model.records(table, seqs, pass_id, ref_id)
    rec5, _, _ = settle.settle_records(table, seqs, idx, rec1)
    words, lens, nmask = pack.pack_reads(seqs)
    assert set(status_of(rec1).tolist()) == {0, 1, 2, 3, 4} and nmask is not None
    return table, words, lens, nmask, rec1, rec5


def settle_direct(eng, table, words, lens, nmask, idx, rec):
    """mrg_a2i_settle on device tensors -> (examined, settled); rec is rewritten in place."""
    from mirge_amd._native import check
    canon_t = np.ascontiguousarray(table.by_pass[0], dtype=np.int32)
    iso_t = np.ascontiguousarray(table.by_pass[8], dtype=np.int32)
    t_words = np.ascontiguousarray(table.words, dtype=np.uint64)
    t_lens = np.ascontiguousarray(table.lens, dtype=np.uint8)
    counts = (C.c_uint64 * 2)()
    n = int(words.shape[1])
    check(eng._lib.mrg_a2i_settle(eng._h, words.data_ptr(), int(words.shape[0]), n, lens.data_ptr(), nmask.data_ptr(), n,
                                  canon_t.ctypes.data, canon_t.shape[0], iso_t.ctypes.data, iso_t.shape[0], t_words.ctypes.data,
                                  t_lens.ctypes.data, t_lens.shape[0], 0, 2, int(idx.shape[0]), idx.data_ptr(), rec.data_ptr(), counts,
                                  None, eng._stream_ptr()))
    return int(counts[0]), int(counts[1])


@pytest.mark.parametrize("n_tied", [1, 63, 64, 65, 70001])
def test_counts_of_tied_rows_among_the_others_and_a_second_call(eng, pool, n_tied):
    import torch
    table, p_words, p_lens, p_nmask, p_rec1, p_rec5 = pool
    rng = np.random.default_rng(n_tied)
    ends = np.nonzero(status_of(p_rec1) == model.ENDS)[0]
    rest = np.nonzero(status_of(p_rec1) != model.ENDS)[0]
    src = rng.permutation(np.concatenate([rng.choice(ends, n_tied), rng.choice(rest, n_tied // 2 + 3)]))
    k = src.size
    dev = eng.device
    words = torch.from_numpy(p_words[:, src].view(np.int64).copy()).to(dev)
    lens = torch.from_numpy(p_lens[src].copy()).to(dev)
    nmask = torch.from_numpy(p_nmask[:, src].view(np.int64).copy()).to(dev)
    idx = torch.arange(k, dtype=torch.int32, device=dev)
    rec = torch.from_numpy(p_rec1[src].copy()).to(dev)
    want = p_rec5[src]
    settled = int((status_of(want) == settle.TIED).sum())
    assert settle_direct(eng, table, words, lens, nmask, idx, rec) == (n_tied, settled)
    got = rec.cpu().numpy()
    assert_same(got, want)
    assert settle_direct(eng, table, words, lens, nmask, idx, rec) == (n_tied - settled, 0)    # a second call: nothing more
    assert np.array_equal(rec.cpu().numpy(), got)


def test_records_out_of_range_are_left_alone(eng, pool):
    """A row of status 1 whose read or target id is no read / target keeps every byte and faults nothing."""
    import torch
    table, p_words, p_lens, p_nmask, p_rec1, p_rec5 = pool
    ends = np.nonzero((status_of(p_rec1) == model.ENDS) & (status_of(p_rec5) == settle.TIED))[0][:6]
    dev = eng.device
    words = torch.from_numpy(p_words.view(np.int64).copy()).to(dev)
    lens, nmask = torch.from_numpy(p_lens.copy()).to(dev), torch.from_numpy(p_nmask.view(np.int64).copy()).to(dev)
    rows = p_rec1[ends].copy()
    ids = ends.astype(np.int32)
    rows[0, 3], rows[1, 3], ids[2] = len(table.names), -1, p_lens.size
    rows[3, 0] &= 0xFFFF            # m = 0 cannot be a tie
    idx, rec = torch.from_numpy(ids).to(dev), torch.from_numpy(rows.copy()).to(dev)
    assert settle_direct(eng, table, words, lens, nmask, idx, rec) == (6, 2)
    got = rec.cpu().numpy()
    assert np.array_equal(got[:4], rows[:4]) and np.array_equal(got[4:], p_rec5[ends[4:]])


# ------------------------------------------------------------------ the command line
TIE_MIRNAS = [("syn-miR-tie-1", "AC" * 11), ("syn-miR-tie-2", "AAG" * 7 + "A"), ("syn-miR-tie-3", "AT" * 11), ("syn-miR-tie-4", "AAC" * 7 + "A")]


def test_annotate_ai_on_a_tie_heavy_world_equals_ai_host(native_lib, tmp_path, monkeypatch):
    """Low-complexity miRNAs whose reads tie between diagonals: the array route settles them on the device and writes what
    the record route writes."""
    with open(os.path.join(ROOT, "tests", "golden", "a2i.json")) as fh:
        golden = json.load(fh)
    golden["libraries"]["mirna"] = [list(golden["libraries"]["mirna"][0]), list(golden["libraries"]["mirna"][1])]
    golden["samples"] = [list(r) for r in golden["samples"]]
    for name, body in TIE_MIRNAS:
        golden["libraries"]["mirna"][0].append(name)
        golden["libraries"]["mirna"][1].append(body)
        for sample in golden["samples"]:
            sample += [body] * 4 + [body[:-2]] * 3 + [body[:-3]] * 3 + ["G" + body[1:-2] + "GG"] * 2
    root, fastqs, _ = golden_layout(golden, tmp_path)
    seen = []
    real = a2i.a_to_i_report_arrays

    def spy(*a, **k):
        timings = k.setdefault("timings", {})
        out = real(*a, **k)
        seen.append(dict(timings))
        return out
    monkeypatch.setattr(a2i, "a_to_i_report_arrays", spy)
    new = run_ai(tmp_path, root, fastqs, "new")
    old = run_ai(tmp_path, root, fastqs, "old", ["--ai-host"])
    assert len(seen) == 1 and seen[0]["tied_rows"] > 0
    for fn in ("a2IEditing.detail.txt", "a2IEditing.report.csv", "a2IEditing.report.newform.csv"):
        assert open(os.path.join(new, fn), "rb").read() == open(os.path.join(old, fn), "rb").read(), fn
