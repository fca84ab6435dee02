"""The array route of `-ai` without a GPU: the model of the alignment kernel (tests/a2i_align_model.py) against
local_pair / judge_align / a2i_editing, and a_to_i_report_arrays + the native detail writer, fed the model's records,
against a_to_i_report and the golden fixture."""
import copy
import io
import json
import os
import random

import numpy as np
import pytest

from mirge_amd import a2i, pack
from tests import a2i_align_model as model
from tests.conftest import ROOT
from tests.test_a2i import check_files

FILES = ("a2IEditing.detail.txt", "a2IEditing.report.csv", "a2IEditing.report.newform.csv")


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "a2i.json")) as fh:
        return json.load(fh)


WORLDS = {"ties": lambda: model.TIE_CASES, "random": model.random_pairs, "isomir": model.isomir_world}
NON_SIMPLE_CAP = 0.10   # on the isomiR-like world: a condition on the input, so the fallback cannot hide the work


@pytest.mark.parametrize("world", sorted(WORLDS))
def test_model_equals_the_python_route_on_every_simple_pair(world):
    pairs = WORLDS[world]()
    simple = edited = judged = 0
    for t, s in pairs:
        status, d, m, verdict, substring, mask = model.align_pair(t, s)
        if status != model.SIMPLE:
            continue
        simple += 1
        la, lb = len(t), len(s)
        assert a2i.local_pair(t, s) == ("-" * max(0, -d) + t + "-" * max(0, d + lb - la),
                                        "-" * max(0, d) + s + "-" * max(0, la - d - lb)), (t, s)
        kept, positions, pos_count, _, _, count_true, seq_true, canonical = a2i.a2i_editing(
            t, [s], [3], "x", io.StringIO(), {s})
        assert bool(verdict) == (seq_true == 1), (t, s)                  # judge_align on local_pair's frame
        assert canonical == (3 if verdict and substring else 0) and bool(substring) == (s in t), (t, s)
        assert positions == ([k + 1 for k in range(32) if mask >> k & 1] if verdict else []), (t, s)
        judged += verdict
        edited += bool(mask)
    share = 1 - simple / len(pairs)
    print("%s: %d pairs, %.1f %% not simple, %d judged True, %d with an edit" % (world, len(pairs), 100 * share, judged, edited))
    assert simple > 0 and judged > 0
    if world == "isomir":
        assert share <= NON_SIMPLE_CAP and edited > 20
    if world == "random":
        assert share > 0.1       # (this world is there for the ties and the indels)


def test_model_statuses_and_edges():
    t = "TGAGGTAGTAGGTTGTATAGTT"
    assert model.align_pair(t, t) == (0, 0, 44, 1, 1, 0)
    assert model.align_pair(t, t[2:])[:4] == (0, 2, 40, 0)
    assert model.align_pair("GC" + "A" * 18 + "TG", "A" * 17)[0] == model.ENDS
    assert model.align_pair("CAGTTCGAGCTATGGACTTCAAGC", "CAGTTCGAGCTAGGACTTCAAGC")[0] == model.GAPPED
    assert model.align_pair("TGCATCGGATCGTACCTGAAGT", "TGCATCGGATCTACCTGAAGT")[0] == model.GAPPED   # the gapped path ties
    assert model.align_pair("AAAA", "CCCC")[0] == model.NOSCORE and model.align_pair("AAAA", "NNNN")[0] == model.NOSCORE
    for bad in ((None, t), ("", t), (t, ""), ("A" * 33, t), (t, "A" * 33), ("ACGN", "ACG")):
        assert model.align_pair(*bad) == (model.UNSUPPORTED, 0, 0, 0, 0, 0)
    assert model.align_pair("AAAAA", "GGGAG")[5] == 0                    # la <= 5: no position is scored
    assert model.align_pair("C" * 26 + "A" + "C" * 5, "C" * 26 + "G" + "C" * 5)[5] == 1 << 26
    assert model.align_pair("C" * 27 + "A" + "C" * 4, "C" * 27 + "G" + "C" * 4)[5] == 0


# ------------------------------------------------------------------ states
class SetGenome:
    """String forms only (as oracle.model.ScanGenome): what a_to_i_report_arrays falls back to."""

    def __init__(self, drop=7):
        self.drop = drop

    def unique_best(self, reads):
        return {r for r in reads if sum(map(ord, r)) % self.drop}

    def exact_hit(self, reads):
        return {r for r in reads if sum(map(ord, r)) % 5 == 0}


def arrays_of(seqDic, mirna_names):
    """seqDic (dict order = array order) -> the host arrays of a run."""
    seqs = list(seqDic)
    at = {n: i for i, n in enumerate(mirna_names)}
    pass_id = np.full(len(seqs), -1, dtype=np.int8)
    ref_id = np.full(len(seqs), -1, dtype=np.int32)
    for i, s in enumerate(seqs):
        annot = seqDic[s]["annot"]
        for p in (0, 8):
            if annot[p + 1] != "":
                pass_id[i], ref_id[i] = p, at[annot[p + 1]]
                break
    words, lens, nmask = pack.pack_reads(seqs)
    quant = np.array([seqDic[s]["quant"] for s in seqs], dtype=np.uint32)
    return seqs, words, lens, nmask, quant, pass_id, ref_id


def both_routes(tmp_path, sample_list, log_dic, seqDic, mirDic, name_seq, merged, removed, mirna_names, genome, env=None,
                monkeypatch=None):
    host, arr = tmp_path / "host", tmp_path / "arrays"
    host.mkdir(exist_ok=True)
    arr.mkdir(exist_ok=True)
    sub = {s: r for s, r in seqDic.items() if r["annot"][1] != "" or r["annot"][9] != ""}
    rows_h = a2i.a_to_i_report(str(host), sample_list, copy.deepcopy(log_dic), sub, mirDic, name_seq, merged, removed, genome)
    seqs, words, lens, nmask, quant, pass_id, ref_id = arrays_of(seqDic, mirna_names)
    npp = [mirna_names] * 9
    table = a2i.target_table(npp, merged, name_seq)
    keep = a2i.keep_mask(quant, pass_id, log_dic)
    idx, rec = model.records(table, seqs, pass_id, ref_id, keep)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    rows_a = a2i.a_to_i_report_arrays(str(arr), sample_list, copy.deepcopy(log_dic), words, lens, nmask, quant, pass_id, idx, rec,
                                      table, mirDic, name_seq, removed, genome)
    assert rows_a == rows_h
    for fn in FILES:
        a, b = open(str(arr / fn), "rb").read(), open(str(host / fn), "rb").read()
        assert a.split(b"\n") == b.split(b"\n"), fn     # (line for line, in the same order)
        assert a == b, fn
    return str(arr), rec


def golden_state(golden):
    st = golden["state"]
    return (golden["sample_list"], {"quantStats": copy.deepcopy(st["quantStats"])}, st["seqDic"], st["mirDic"],
            golden["mirNameSeqDic"], golden["mirMergedNameDic"], golden["removedMiRNAList"], golden["libraries"]["mirna"][0])


@pytest.mark.parametrize("threads", [1, 5, 16])
def test_report_from_arrays_equals_the_record_route_and_the_golden(golden, native_lib, oracle_lib, tmp_path, monkeypatch, threads):
    from oracle import model as omodel
    genome = omodel.ScanGenome(omodel.Library(*golden["libraries"]["genome"]))
    out, rec = both_routes(tmp_path, *golden_state(golden), genome,
                           env={"MIRGE_AMD_TABLE_THREADS": str(threads), "MIRGE_AMD_A2I_RUN_BLOCKS": "3"}, monkeypatch=monkeypatch)
    check_files(golden, out)
    status = rec[:, 0] & 0xFF
    assert (status == 0).sum() > 100 and (status != 0).any()    # the fixture holds both kinds


def synthetic_state(kind, seed):
    """A world of 30 miRNAs x 2 samples.  kind 'none': every read is simple; 'all': every (miRNA, sample) selection holds
    a read the kernel leaves to the host (a tie, a deletion that wins, an N-free read of 33 nt)."""
    rnd = random.Random(seed)
    names, name_seq, seqDic, mirDic = [], {}, {}, {}
    for t in range(30):
        name = "syn-miR-%d" % t
        target = "".join(rnd.choice("ACGT") for _ in range(rnd.randint(20, 24)))
        if "A" not in target[:10]:
            target = "A" + target[1:]
        names.append(name)
        name_seq[name] = target
        reads = {target: 0}
        for _ in range(8):
            s = list(target[rnd.randint(0, 1):len(target) - rnd.randint(0, 2)])
            if rnd.random() < 0.7:
                k = rnd.choice([i for i, ch in enumerate(s[:12]) if ch == "A"] or [0])
                s[k] = "G"
            reads["".join(s) + rnd.choice(["", "T", "TA"])] = 8
        if kind == "all":
            reads[target[:12] + target[13:] + "ACGTACGTAC"[:rnd.randint(0, 3)]] = 8     # a deletion: gapped or tied
            reads[target + "ACGTACGTACGTA"[:33 - len(target)]] = 8                       # 33 nt
        total = [0, 0]
        for s, p in reads.items():
            if kind == "none" and model.align_pair(target, s)[0] != model.SIMPLE:
                continue
            q = [rnd.randint(3, 60), rnd.randint(3, 60)]
            annot = [1] + [""] * 9
            annot[p + 1] = name
            seqDic[s] = {"quant": q, "annot": annot, "length": len(s)}
            total = [total[0] + q[0], total[1] + q[1]]
        mirDic[name] = {"quant": total, "iscan": total}
    log_dic = {"quantStats": [{"mirnaReadsFiltered": 20000}, {"mirnaReadsFiltered": 30000}]}
    return ["s1.fastq", "s2.fastq"], log_dic, seqDic, mirDic, name_seq, {}, ["syn-miR-3"], names


@pytest.mark.parametrize("kind", ["none", "all"])
def test_worlds_where_no_group_or_every_group_needs_the_host(kind, native_lib, tmp_path):
    state = synthetic_state(kind, 11)
    out, rec = both_routes(tmp_path, *state, SetGenome())
    status = rec[:, 0] & 0xFF
    seqDic, names = state[2], state[7]
    if kind == "none":
        assert (status == 0).all()
    else:
        group = np.array([names.index(r["annot"][1] or r["annot"][9]) for r in seqDic.values()])
        assert all((status[group == g] != 0).any() for g in range(len(names)))
    assert len(open(os.path.join(out, "a2IEditing.report.csv")).read().split("\n")) > 5
    assert os.path.getsize(os.path.join(out, "a2IEditing.detail.txt")) > 10000


def test_target_table_scales_with_the_library_and_marks_what_the_kernel_cannot_take():
    names = ["a", "b", "c", "d", "e"]
    merged = {"a": "a/b", "b": "a/b"}
    seqs = {"a/b": "ACGTACGTACGTACGTACGT", "c": "ACGN" * 5, "d": "A" * 33}
    t = a2i.target_table([names] * 9, merged, seqs)
    assert t.names == ["a/b", "c", "d", "e"] and t.by_pass[0].tolist() == [0, 0, 1, 2, 3] == t.by_pass[8].tolist()
    assert t.lens.tolist() == [20, 0, 0, 0] and t.seqs == ["ACGTACGTACGTACGTACGT", "ACGN" * 5, "A" * 33, None]
    assert pack.unpack_reads(t.words[None, :1], t.lens[:1]) == ["ACGTACGTACGTACGTACGT"]


def test_detail_writer_refuses_rows_that_do_not_fit(native_lib, tmp_path):
    from mirge_amd._native import MirgeAmdError
    words, lens, nmask = pack.pack_reads(["ACGTACGT", "ACGNACGTAA"])
    args = dict(block_off=[0, 2], block_group=[0], block_frame=[[1, 2]], block_text=[None], group_names=["m"],
                group_targets=["ACGTACGT"], row_read=[0, 1], row_count=[4, 5], row_flags=[3, 1], row_d=[0, -1])
    p = str(tmp_path / "d.txt")
    assert a2i.write_a2i_detail(p, words, lens, nmask, **args) == 5 + 2 + 2 + 1
    assert open(p).read() == ("Canonical_Seq of m: ACGTACGT\nseqList size is: 2, 2\n-ACGTACGT--\t4\tTrue\nACGNACGTAA-\t5\tTrue\n"
                              "****************\nretained seqList size is: 1\n-ACGTACGT--\t4\tTrue\nACGNACGTAA-\t5\tTrue\n"
                              "****************\nretained sequences after filering are:\n-ACGTACGT--\t4\tTrue\n")
    with pytest.raises(MirgeAmdError):
        a2i.write_a2i_detail(p, words, lens, nmask, **dict(args, row_d=[0, -2]))
    with pytest.raises(MirgeAmdError):
        a2i.write_a2i_detail(p, words, lens, nmask, **dict(args, row_read=[0, 2]))
    assert a2i.write_a2i_detail(p, words, lens, nmask, **dict(args, block_text=["x\ny\n"])) == 2 and open(p).read() == "x\ny\n"
