"""`-ai` on the GPU: mrg_a2i_align (csrc/a2i_align.hip) against its model (tests/a2i_align_model.py) field by field, the
array forms of the genome filters against the string forms, and `annotate -ai` with and without --ai-host."""
import json
import os
import random
import types

import numpy as np
import pytest

from mirge_amd import a2i, pack
from tests import a2i_align_model as model
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu

FIELDS = ("status", "verdict", "substring", "m", "d", "mask", "target")


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "a2i.json")) as fh:
        return json.load(fh)


@pytest.fixture(scope="module")
def eng(native_lib):
    from mirge_amd.engine import Engine
    return Engine(0)


def decode(rec):
    f = rec[:, 0]
    return np.stack([f & 0xFF, (f >> 8) & 1, (f >> 9) & 1, (f >> 16) & 0xFFFF, rec[:, 1], rec[:, 2], rec[:, 3]], axis=1)


def world_of(pairs, name_seq_extra=None):
    """Every distinct target becomes a library entry; read i is claimed by pass 0 (even i) or 8 (odd i) on its entry."""
    targets = list(dict.fromkeys(t for t, _ in pairs))
    at = {t: i for i, t in enumerate(targets)}
    names = ["t%d" % i for i in range(len(targets))]
    name_seq = {n: t for n, t in zip(names, targets) if t is not None}
    table = a2i.target_table([names] * 9, {}, name_seq)
    seqs = [s for _, s in pairs]
    pass_id = np.array([0 if i % 2 == 0 else 8 for i in range(len(pairs))], dtype=np.int8)
    ref_id = np.array([at[t] for t, _ in pairs], dtype=np.int32)
    return table, seqs, pass_id, ref_id


def assert_same(got, want, pairs=None):
    assert got.shape == want.shape
    if not np.array_equal(got, want):
        a, b = decode(got), decode(want)
        row = int(np.nonzero((a != b).any(axis=1))[0][0])
        raise AssertionError("row %d %r: kernel %s, model %s" % (row, pairs[row] if pairs else None, dict(zip(FIELDS, a[row].tolist())),
                                                               dict(zip(FIELDS, b[row].tolist()))))


def run_pairs(eng, pairs, W=None, **kw):
    table, seqs, pass_id, ref_id = world_of(pairs)
    words, lens, nmask = pack.pack_reads(seqs, W)
    idx, rec = eng.a2i_align(table, words, lens, nmask, pass_id, ref_id, **kw)
    w_idx, w_rec = model.records(table, seqs, pass_id, ref_id, **{k: v for k, v in kw.items() if k in ("from_base", "to_base")})
    assert np.array_equal(idx, w_idx)
    assert_same(rec, w_rec, pairs)
    return rec


@pytest.mark.parametrize("world", ["ties", "random", "isomir"])
def test_kernel_equals_the_model_on_the_three_worlds(eng, world):
    pairs = {"ties": lambda: model.TIE_CASES, "random": model.random_pairs, "isomir": model.isomir_world}[world]()
    rec = run_pairs(eng, pairs)
    status = rec[:, 0] & 0xFF
    assert (status == 0).any()
    if world != "isomir":
        assert (status == 1).any() and (status == 2).any()
    if world == "isomir":
        assert (status != 0).mean() <= 0.10
        run_pairs(eng, pairs[:300], from_base="C", to_base="T")


def test_every_length_pair_at_every_diagonal(eng):
    rnd = random.Random(5)
    other = {"A": "C", "C": "G", "G": "T", "T": "A"}
    pairs = []
    for la in (1, 5, 6, 31, 32):
        for lb in (1, 5, 6, 31, 32):
            t = "".join(rnd.choice("ACGT") for _ in range(la))
            for d in range(-(lb - 1), la):
                s = [t[c + d] if 0 <= c + d < la else rnd.choice("ACGT") for c in range(lb)]
                pairs.append((t, "".join(s)))
                inside = [c for c in range(lb) if 0 <= c + d < la]
                c = rnd.choice(inside)
                s[c] = "G" if t[c + d] == "A" else other[s[c]]      # an edit where the target holds A, else a mismatch
                pairs.append((t, "".join(s)))
    rec = run_pairs(eng, pairs)
    f = decode(rec)
    simple = f[f[:, 0] == 0]
    assert len(pairs) == 1450 and set(range(-26, 27)) <= set(simple[:, 4].tolist())     # (a shorter overlap ties by chance)
    assert simple[:, 1].any() and simple[:, 2].any() and (simple[:, 5] != 0).any()


def test_mask_edges_and_n_in_the_read(eng):
    t22 = "TGAGGTAGTAGGTTGTATAGTT"
    cases = [   # (target, read) -> (status, d, m, verdict, substring, mask); None: the model alone decides
        (("CACTT", "CGCTT"), (0, 0, 7, 1, 0, 0)),                       # la <= 5: an empty mask, whatever the read shows
        (("AAAAA", "AAAAA"), (0, 0, 10, 1, 1, 0)),
        (("ACTTGC", "GCTTGC"), (0, 0, 10, 1, 0, 1)),                    # la = 6: position 0 alone is scored
        (("CACTTGC", "CGCTTGC"), (0, 0, 11, 1, 0, 2)),
        (("C" * 26 + "A" + "C" * 5, "C" * 26 + "G" + "C" * 5), (0, 0, 61, 1, 0, 1 << 26)),   # la = 32: bit 26 is the last
        (("C" * 27 + "A" + "C" * 4, "C" * 27 + "G" + "C" * 4), (0, 0, 61, 1, 0, 0)),
        (("A" * 32, "G" * 32), (3, 0, 0, 0, 0, 0)),
        (("A" * 32, "A" * 16 + "G" * 16), (1, 0, 32, 0, 0, 0)),
        ((t22, t22[:4] + "N" + t22[5:]), (0, 0, 41, 1, 0, 0)),          # an N costs a match ...
        ((t22, "N" + t22[1:]), (0, 0, 42, 1, 0, 0)),
        ((t22, t22[:-1] + "N"), (0, 0, 42, 1, 0, 0)),
        ((t22, "N" * 22), (3, 0, 0, 0, 0, 0)),                          # ... and N alone scores nothing
        ((t22, "NN" + t22), (0, -2, 44, 0, 0, 0)),
        ((t22, t22[:2] + "G" + t22[3:9] + "N" + t22[10:]), (0, 0, 38, 0, 0, 4)),
        ((t22, t22[:2] + "N" + t22[3:]), (0, 0, 41, 1, 0, 0)),          # an N where the target holds A is no G
        (("ACGTACGT", "ACNTACGT"), (0, 0, 13, 1, 0, 0)),
        (("AAAAA", "GGGAG"), None), (("AAAAAA", "GAAAAA"), None)]
    f = decode(run_pairs(eng, [c[0] for c in cases]))
    for row, (pair, want) in zip(f.tolist(), cases):
        if want is not None:
            status, verdict, substring, m, d, mask = row[:6]
            assert (status, d, m, verdict, substring, mask) == want, pair


def test_targets_the_kernel_cannot_take(eng):
    names = ["ok", "with_n", "long", "missing", "merged_a", "merged_b"]
    name_seq = {"ok": "TGAGGTAGTAGGTTGTATAGTT", "with_n": "TGAGGTAGTANGTTGTATAGTT", "long": "ACGT" * 9, "fam": "ACGTTGCAACGTTGCAACGT"}
    table = a2i.target_table([names] * 9, {"merged_a": "fam", "merged_b": "fam"}, name_seq)
    assert table.names == ["ok", "with_n", "long", "missing", "fam"] and table.lens.tolist() == [22, 0, 0, 0, 20]
    seqs = ["TGAGGTAGTAGGTTGTATAGTT"] * 4 + ["ACGTTGCAACGTTGCAACGT"] * 2 + ["TGAGGTAGTAGGTTGTATAGTT"] * 3 + ["A" * 40]
    ref_id = np.array([0, 1, 2, 3, 4, 5, 6, -1, 0, 0], dtype=np.int32)       # 6 and -1: no such entry
    pass_id = np.array([0, 8, 0, 8, 0, 8, 0, 8, 3, 0], dtype=np.int8)        # read 8 belongs to another pass
    words, lens, nmask = pack.pack_reads(seqs)
    assert words.shape[0] == 2
    idx, rec = eng.a2i_align(table, words, lens, nmask, pass_id, ref_id)
    w_idx, w_rec = model.records(table, seqs, pass_id, ref_id)
    assert idx.tolist() == [0, 1, 2, 3, 4, 5, 6, 7, 9] == w_idx.tolist()
    assert_same(rec, w_rec)
    f = decode(rec)
    assert f[:, 0].tolist() == [0, 4, 4, 4, 0, 0, 4, 4, 4] and f[:, 6].tolist() == [0, 1, 2, 3, 4, 4, -1, -1, 0]
    assert f[4].tolist()[:5] == [0, 1, 1, 40, 0]


def test_bad_tables_are_refused_before_any_launch(eng):
    from mirge_amd._native import MirgeAmdError
    table = a2i.target_table([["a", "b"]] * 9, {}, {"a": "ACGTACGTACGTACGTACGT", "b": "ACGTACGTACGTACGTACTT"})
    words, lens, nmask = pack.pack_reads(["ACGTACGTACGTACGTACGT"])
    args = (words, lens, nmask, np.zeros(1, np.int8), np.zeros(1, np.int32))
    for change in (dict(by_pass={0: np.array([0, 2], np.int32), 8: table.by_pass[8]}),
                   dict(by_pass={0: np.array([0, -2], np.int32), 8: table.by_pass[8]}),
                   dict(lens=np.array([20, 33], np.uint8)), dict(lens=np.array([20, 19], np.uint8))):
        bad = a2i.TargetTable(**{**dict(names=table.names, seqs=table.seqs, words=table.words, lens=table.lens,
                                        by_pass=table.by_pass), **change})
        with pytest.raises(MirgeAmdError):
            eng.a2i_align(bad, *args)
    with pytest.raises(MirgeAmdError):
        eng.a2i_align(table, *args, canon_pass=8)
    idx, rec = eng.a2i_align(table, *args)
    assert idx.tolist() == [0] and decode(rec)[0].tolist() == [0, 1, 1, 40, 0, 0, 0]


@pytest.fixture(scope="module")
def pool():
    """300 distinct pairs and the model's fields for each, computed once."""
    pairs = model.isomir_world(n_targets=25, reads_per_target=12, seed=77)
    table, seqs, _, ref_id = world_of(pairs)
    fields = np.array([model.pack_record(model.align_pair(t, s), int(ref_id[i])) for i, (t, s) in enumerate(pairs)], dtype=np.int64)
    words, lens, nmask = pack.pack_reads(seqs)
    return table, words, lens, ref_id, fields.astype(np.int32)


@pytest.mark.parametrize("n_pairs", [1, 63, 64, 65, 70001])
@pytest.mark.parametrize("with_keep", [False, True])
def test_pair_counts_and_selection_order(eng, pool, n_pairs, with_keep):
    table, p_words, p_lens, p_ref, p_rec = pool
    rng = np.random.default_rng(n_pairs + with_keep)
    # reads of other passes and unclaimed reads between the selected ones; with keep, twice as many candidates
    n_sel = n_pairs * (2 if with_keep else 1)
    n = n_sel + n_sel // 2 + 3
    slot = rng.permutation(n)[:n_sel]
    pass_id = rng.choice(np.array([-1, 1, 3, 7], dtype=np.int8), n)
    pass_id[slot] = rng.choice(np.array([0, 8], dtype=np.int8), n_sel)
    src = rng.integers(0, p_lens.size, n)
    keep = None
    chosen = np.sort(slot)
    if with_keep:
        keep = np.ones(n, dtype=bool)
        keep[rng.permutation(slot)[:n_sel - n_pairs]] = False
        other = np.nonzero((pass_id != 0) & (pass_id != 8))[0]
        keep[other[::3]] = False                    # (the keep byte of a read of another pass means nothing)
        chosen = np.array([i for i in chosen if keep[i]], dtype=np.int64)
    idx, rec = eng.a2i_align(table, p_words[:, src], p_lens[src], None, pass_id, p_ref[src], keep)
    assert idx.dtype == np.uint32 and np.array_equal(idx, chosen)        # array order
    if not with_keep:
        assert idx.size == n_pairs
    assert_same(rec, p_rec[src[chosen]])


def test_timings_and_device_tensors(eng, pool):
    import torch
    table, p_words, p_lens, p_ref, p_rec = pool
    n = p_lens.size
    dev = eng.device
    pass_id = np.where(np.arange(n) % 3 == 0, 8, 0).astype(np.int8)
    timings = {}
    idx, rec = eng.a2i_align(table, torch.from_numpy(p_words.view(np.int64)).to(dev), torch.from_numpy(p_lens).to(dev), None,
                             torch.from_numpy(pass_id).to(dev), torch.from_numpy(p_ref).to(dev),
                             torch.from_numpy(np.ones(n, np.uint8)).to(dev), timings=timings)
    assert idx.tolist() == list(range(n)) and 0 < timings["kernel_ms"] <= timings["align_call_ms"]
    assert_same(rec, p_rec)


def test_array_genome_masks_equal_the_string_forms(eng, golden):
    from mirge_amd.index import FmIndex
    names, seqs = golden["libraries"]["genome"]
    keys = []
    for n, s in zip(names, seqs):
        eng.add_library("a2i-genome:" + n, FmIndex.build([n], [s]))
        keys.append("a2i-genome:" + n)
    gpu = a2i.EngineGenome(eng, keys)
    reads = [s for s, r in golden["state"]["seqDic"].items() if r["annot"][1] != "" or r["annot"][9] != ""]
    chrom = seqs[0]
    reads += ["ACGT" * 6, "TTTTTTTTTTTTTTTTTTTTTT", chrom[100:140], a2i.revcomp(chrom[300:322]), chrom[500:510] + "N" + chrom[511:524],
              chrom[40:60]]
    reads = list(dict.fromkeys(reads))
    words, lens, nmask = pack.pack_reads(reads)
    assert words.shape[0] == 2 and nmask is not None
    for which in ("unique_best", "exact_hit"):
        want = getattr(gpu, which)(reads)
        got = getattr(gpu, which + "_mask")(words, lens, nmask)
        assert got.dtype == bool and {r for r, g in zip(reads, got) if g} == want
        assert 0 < len(want) < len(reads)


# ------------------------------------------------------------------ the command line
def golden_layout(golden, tmp_path, long_entry=False):
    from mirge_amd import build_index, synth
    libs = {k: (list(v[0]), list(v[1])) for k, v in golden["libraries"].items()}
    samples = [list(r) for r in golden["samples"]]
    long_read = None
    if long_entry:   # a miRNA entry long enough for a read beyond 255 nt, which only the isomiR pass can claim
        rnd = random.Random(9)
        body = "".join(rnd.choice("ACGT") for _ in range(300))
        libs["mirna"][0].append("syn-miR-9999-5p")
        libs["mirna"][1].append(body)
        flip = {"A": "C", "C": "G", "G": "T", "T": "A"}
        long_read = flip[body[9]] + body[10:270] + flip[body[270]] + flip[body[271]]
        for s in samples:
            s += [long_read] * 2
    ns = types.SimpleNamespace(libs={k: tuple(v) for k, v in libs.items()}, merges=golden["merges"])
    root = str(tmp_path / "libs")
    synth.SynthLibraries.write_layout(ns, root, species="syn", db="miRBase")
    gfa = os.path.join(root, "syn", "index.Libs", "syn_genome.fa")
    longest = max(len(s) for s in libs["genome"][1])
    assert build_index.main([gfa, "--max-bases", str(longest + 10)]) == 0
    os.remove(gfa)
    with open(os.path.join(root, "syn", "annotation.Libs", "syn_miRNAs_in_repetitive_element_miRBase.csv"), "w") as fh:
        for n in golden["removedMiRNAList"]:
            fh.write("%s,x\n" % n)
    fastqs = []
    for name, reads in zip(golden["sample_list"], samples):
        p = str(tmp_path / name)
        with open(p, "w") as fh:
            for k, r in enumerate(reads):
                fh.write("@r%d\n%s\n+\n%s\n" % (k, r, "I" * len(r)))
        fastqs.append(p)
    return root, fastqs, long_read


def run_ai(tmp_path, root, fastqs, label, extra=()):
    from mirge_amd import cli
    out = tmp_path / label
    out.mkdir()
    res = cli.annotate_main(cli.build_parser().parse_args(
        ["annotate", "-s"] + fastqs + ["-lib", root, "-sp", "syn", "-o", str(out), "-ai"] + list(extra)))
    return res["outdir"]


def test_annotate_ai_writes_the_same_files_on_both_routes(golden, native_lib, tmp_path, monkeypatch):
    from mirge_amd import columnar
    from tests.test_a2i import check_files
    root, fastqs, _ = golden_layout(golden, tmp_path)
    calls = []
    real_arrays, real_records, real_subset = a2i.a_to_i_report_arrays, a2i.a_to_i_report, columnar.read_subset
    monkeypatch.setattr(a2i, "a_to_i_report_arrays", lambda *a, **k: calls.append("arrays") or real_arrays(*a, **k))
    monkeypatch.setattr(a2i, "a_to_i_report", lambda *a, **k: calls.append("records") or real_records(*a, **k))
    monkeypatch.setattr(columnar, "read_subset", lambda *a, **k: calls.append("subset") or real_subset(*a, **k))
    new = run_ai(tmp_path, root, fastqs, "new")
    assert calls == ["arrays"]                      # no record per read is built
    old = run_ai(tmp_path, root, fastqs, "old", ["--ai-host"])
    assert calls == ["arrays", "subset", "records"]
    for fn in ("a2IEditing.detail.txt", "a2IEditing.report.csv", "a2IEditing.report.newform.csv"):
        assert open(os.path.join(new, fn), "rb").read() == open(os.path.join(old, fn), "rb").read(), fn
    check_files(golden, new)


def test_annotate_ai_with_a_long_mirna_read_takes_the_record_route(golden, native_lib, tmp_path, monkeypatch):
    root, fastqs, long_read = golden_layout(golden, tmp_path, long_entry=True)
    assert len(long_read) == 263
    calls = []
    monkeypatch.setattr(a2i, "a_to_i_report_arrays", lambda *a, **k: calls.append("arrays"))
    monkeypatch.setattr(a2i, "a_to_i_report", lambda outdir, samples, log, sub, *a, **k: calls.append(("records", long_read in sub)))
    run_ai(tmp_path, root, fastqs, "new")
    run_ai(tmp_path, root, fastqs, "old", ["--ai-host"])
    assert calls == [("records", True), ("records", True)]
