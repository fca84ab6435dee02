"""Tied ungapped alignments of `-ai` without a GPU: the model of mrg_a2i_settle (tests/a2i_settle_model.py) against
local_pair / judge_align / a2i_editing on every pair it settles, the cap on what it may leave unsettled,
a_to_i_report_arrays on records that hold status 5 against the same rows as status 1 and against a_to_i_report, and the
argument checks of the entry point."""
import copy
import ctypes as C
import io
import os
import random

import numpy as np
import pytest

from mirge_amd import a2i
from tests import a2i_align_model as model
from tests import a2i_settle_model as settle
from tests.test_a2i_arrays import FILES, SetGenome, arrays_of

WORLDS = {"ties": lambda: model.TIE_CASES, "random": model.random_pairs, "random99": lambda: model.random_pairs(6000, seed=99),
          "isomir": lambda: model.isomir_world(600, 20, 7), "named": lambda: [(t, s) for t, s, _ in settle.COUNTEREXAMPLES]}
UNSETTLED_CAP = 13      # of the 133 pairs of status 1 of isomir_world(600, 20, 7): 10 %, so the fallback cannot hide the work
_fields = {}


def world_fields(world):
    """[(target, read, align_pair's fields, settle_pair's fields)], computed once per world."""
    if world not in _fields:
        _fields[world] = [(t, s, model.align_pair(t, s), settle.settle_pair(t, s)) for t, s in WORLDS[world]()]
    return _fields[world]


@pytest.mark.parametrize("world", sorted(WORLDS))
def test_every_settled_pair_equals_the_python_route(world):
    tied = judged = edited = 0
    for t, s, before, after in world_fields(world):
        if after[0] != settle.TIED:
            assert after == before, (t, s)          # what the rule does not claim keeps its fields
            continue
        assert before[0] == model.ENDS and before[2] == after[2], (t, s)
        tied += 1
        status, d, m, verdict, substring, mask = after
        la, lb = len(t), len(s)
        assert a2i.local_pair(t, s) == ("-" * max(0, -d) + t + "-" * max(0, d + lb - la),
                                        "-" * max(0, d) + s + "-" * max(0, la - d - lb)), (t, s)
        assert bool(verdict) == a2i.judge_align(*a2i.local_pair(t, s)), (t, s)
        kept, positions, pos_count, _, _, count_true, seq_true, canonical = a2i.a2i_editing(t, [s], [3], "x", io.StringIO(), {s})
        assert bool(verdict) == (seq_true == 1), (t, s)
        assert canonical == (3 if verdict and substring else 0) and bool(substring) == (s in t), (t, s)
        assert positions == ([k + 1 for k in range(32) if mask >> k & 1] if verdict else []), (t, s)
        judged += verdict
        edited += bool(mask and verdict)
    print("%s: %d pairs, %d settled, %d judged True, %d with an edit" % (world, len(WORLDS[world]()), tied, judged, edited))
    assert tied > 0
    if world in ("random", "random99"):
        assert tied > 1000 and judged > 0


def test_the_named_pairs_need_the_listing_rule():
    """Eligibility alone answers 10, 2 and 16: the passed-along cells of the last row / column end pairwise2's listing."""
    for t, s, d in settle.COUNTEREXAMPLES:
        assert settle.settle_pair(t, s)[:2] == (settle.TIED, d), (t, s)
    assert settle.settle_pair("GC" + "A" * 18 + "TG", "A" * 17)[:3] == (settle.TIED, 3, 34)     # the run ending furthest along wins
    assert settle.settle_pair("A", "AAAA")[:3] == (settle.TIED, -3, 2)
    assert settle.settle_pair("AAAA", "A")[:3] == (settle.TIED, 3, 2)
    t = "TGCATCGGATCGTACCTGAAGT"
    assert settle.settle_pair(t, "TGCATCGGATCTACCTGAAGT") == model.align_pair(t, "TGCATCGGATCTACCTGAAGT")   # gapped: untouched


def test_cap_on_the_unsettled_share():
    rows = world_fields("isomir")
    ends = [r for r in rows if r[2][0] == model.ENDS]
    left = [r for r in ends if r[3][0] != settle.TIED]
    print("isomir_world(600, 20, 7): %d pairs of status 1, %d left unsettled" % (len(ends), len(left)))
    assert len(ends) == 133 and len(left) <= UNSETTLED_CAP


# ------------------------------------------------------------------ the report from records that hold status 5
def tie_heavy_state(seed, with_host_reads):
    """24 miRNAs that repeat a unit of 2-4 nt (one base changed in every other one) x 3 samples, 7+ reads per miRNA, every
    read in every sample; every miRNA has a tied read.
    with_host_reads: every third miRNA also holds a read only the host settles (a deletion that wins or ties, 33 nt)."""
    rnd = random.Random(seed)
    names, name_seq, seqDic, mirDic = [], {}, {}, {}
    while len(names) < 24:
        unit = "A" + "".join(rnd.choice("ACGT") for _ in range(rnd.randint(1, 3)))
        target = list((unit * 12)[:rnd.randint(20, 24)])
        if rnd.random() < 0.5:
            target[rnd.randrange(len(target))] = rnd.choice("CGT")
        target = "".join(target)
        if "A" not in target[:10] or target in name_seq.values():
            continue
        reads, tied = {target: 0}, 0
        for _ in range(60):
            s = list(target[rnd.randint(0, 2):len(target) - rnd.randint(0, 3)])
            if rnd.random() < 0.7:
                k = rnd.choice([i for i, ch in enumerate(s[:12]) if ch == "A"] or [0])
                s[k] = "G"
            s = "".join(s) + rnd.choice(["", "T", "TA", "A"])
            if s in reads or s in seqDic:
                continue
            status = settle.settle_pair(target, s)[0]
            if status in (model.SIMPLE, settle.TIED) and (status == settle.TIED or len(reads) - tied < 5):
                reads[s] = 8
                tied += status == settle.TIED
            if len(reads) >= 8 and tied >= 2:
                break
        if tied == 0 or settle.settle_pair(target, target)[0] not in (model.SIMPLE, settle.TIED):
            continue
        name = "syn-miR-%d" % len(names)
        if with_host_reads and len(names) % 3 == 0:
            reads[target[:12] + target[13:] + "GT"] = 8
            reads[target + "ACGTACGTACGTA"[:33 - len(target)]] = 8
        names.append(name)
        name_seq[name] = target
        total = [0, 0, 0]
        for s, p in reads.items():
            q = [rnd.randint(3, 60) for _ in range(3)]
            annot = [1] + [""] * 9
            annot[p + 1] = name
            seqDic[s] = {"quant": q, "annot": annot, "length": len(s)}
            total = [a + b for a, b in zip(total, q)]
        mirDic[name] = {"quant": total, "iscan": total}
    log_dic = {"quantStats": [{"mirnaReadsFiltered": 20000}, {"mirnaReadsFiltered": 30000}, {"mirnaReadsFiltered": 25000}]}
    return ["s1.fastq", "s2.fastq", "s3.fastq"], log_dic, seqDic, mirDic, name_seq, {}, ["syn-miR-3"], names


def three_reports(tmp_path, state):
    """a_to_i_report, and a_to_i_report_arrays on the model's records with and without status 5 -> the two timings."""
    sample_list, log_dic, seqDic, mirDic, name_seq, merged, removed, names = state
    genome = SetGenome()
    dirs = {k: tmp_path / k for k in ("host", "tied", "ends")}
    for d in dirs.values():
        d.mkdir()
    rows_h = a2i.a_to_i_report(str(dirs["host"]), sample_list, copy.deepcopy(log_dic), seqDic, mirDic, name_seq, merged, removed,
                               genome)
    seqs, words, lens, nmask, quant, pass_id, ref_id = arrays_of(seqDic, names)
    table = a2i.target_table([names] * 9, merged, name_seq)
    keep = a2i.keep_mask(quant, pass_id, log_dic)
    idx, rec1 = model.records(table, seqs, pass_id, ref_id, keep)
    rec5, examined, settled = settle.settle_records(table, seqs, idx, rec1)
    assert examined == int(((rec1[:, 0] & 0xFF) == model.ENDS).sum()) and settled == int(((rec5[:, 0] & 0xFF) == settle.TIED).sum())
    assert settled > 0 and np.array_equal(rec1[(rec5[:, 0] & 0xFF) != settle.TIED], rec5[(rec5[:, 0] & 0xFF) != settle.TIED])
    timings = {}
    for key, rec in (("tied", rec5), ("ends", rec1)):
        timings[key] = {}
        rows = a2i.a_to_i_report_arrays(str(dirs[key]), sample_list, copy.deepcopy(log_dic), words, lens, nmask, quant, pass_id, idx,
                                        rec, table, mirDic, name_seq, removed, genome, timings=timings[key])
        assert rows == rows_h
    for fn in FILES:
        want = open(str(dirs["host"] / fn), "rb").read()
        assert open(str(dirs["tied"] / fn), "rb").read() == want, fn
        assert open(str(dirs["ends"] / fn), "rb").read() == want, fn
    assert os.path.getsize(str(dirs["host"] / FILES[0])) > 10000 and len(rows_h) > 3
    assert timings["tied"]["tied_rows"] == settled and timings["ends"]["tied_rows"] == 0
    return timings["tied"], timings["ends"]


def test_report_with_status_5_sends_fewer_blocks_to_the_host(native_lib, tmp_path):
    tied, ends = three_reports(tmp_path, tie_heavy_state(21, with_host_reads=True))
    assert tied["blocks"] == ends["blocks"] == 72
    assert 0 < tied["host_blocks"] < ends["host_blocks"] == 72


def test_report_with_status_5_needs_no_host_block_where_every_block_did(native_lib, tmp_path):
    tied, ends = three_reports(tmp_path, tie_heavy_state(22, with_host_reads=False))
    assert tied["blocks"] == ends["blocks"] == 72
    assert tied["host_blocks"] == 0 and ends["host_blocks"] == 72


# ------------------------------------------------------------------ the entry point's argument checks
def test_settle_entry_point_names_what_is_wrong_and_needs_a_context(native_lib):
    from mirge_amd import _native
    L = native_lib
    assert a2i.ST_TIED == settle.TIED == 5
    buf = np.zeros(16, dtype=np.uint64)
    p = buf.ctypes.data
    counts = (C.c_uint64 * 2)()
    canon = np.array([0, 1], dtype=np.int32)
    iso = np.array([1, -1], dtype=np.int32)
    words = np.array([0x1B, 0x1B1B], dtype=np.uint64)
    lens = np.array([3, 7], dtype=np.uint8)

    def call(ctx=None, reads=p, W=1, canon=canon, iso=iso, words=words, lens=lens, counts=counts, from_base=0, idx=p, rec=p):
        return L.mrg_a2i_settle(ctx, reads, W, 4, p, None, 4, None if canon is None else canon.ctypes.data, 2,
                                None if iso is None else iso.ctypes.data, 2, None if words is None else words.ctypes.data,
                                None if lens is None else lens.ctypes.data, 2, from_base, 2, 3, idx, rec, counts, None, None)
    for kw in (dict(counts=None), dict(reads=None), dict(idx=None), dict(rec=None), dict(canon=None), dict(iso=None),
               dict(words=None), dict(lens=None)):
        assert call(**kw) == _native.MRG_ERR_ARG, kw
        assert b"mrg_a2i_settle: null" in L.mrg_last_error(), kw
    assert call(W=3) == _native.MRG_ERR_ARG and b"words_per_read" in L.mrg_last_error()
    assert call(from_base=4) == _native.MRG_ERR_ARG and b"from_base" in L.mrg_last_error()
    assert call(rec=p + 8) == _native.MRG_ERR_ARG and b"16-byte" in L.mrg_last_error()
    assert call(canon=np.array([0, 2], dtype=np.int32)) == _native.MRG_ERR_ARG
    assert b"mrg_a2i_settle: entry 1 of the canonical table names target 2 of 2" in L.mrg_last_error()
    assert call(iso=np.array([-2, 0], dtype=np.int32)) == _native.MRG_ERR_ARG
    assert b"mrg_a2i_settle: entry 0 of the isomiR table names target -2" in L.mrg_last_error()
    assert call(lens=np.array([3, 33], dtype=np.uint8)) == _native.MRG_ERR_ARG
    assert b"mrg_a2i_settle: target 1 has 33 bases (at most 32)" in L.mrg_last_error()
    assert call(lens=np.array([2, 7], dtype=np.uint8)) == _native.MRG_ERR_ARG and b"beyond its length" in L.mrg_last_error()
    # nothing wrong with the arguments: the rows are settled on the device or not at all
    assert call() == _native.MRG_ERR_ARG and b"mrg_a2i_settle: null context" in L.mrg_last_error()
    import torch
    if not torch.cuda.is_available():
        ctx = C.c_void_p()
        assert L.mrg_ctx_create(0, C.byref(ctx)) == _native.MRG_ERR_NO_DEVICE and not ctx.value
