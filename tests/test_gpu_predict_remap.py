"""Predict mode's second mapping on the GPU (-m gpu): mrg_predict_trim_reads against bowtie.trim + pack.pack_reads and
mrg_predict_remap_rows against the model (tests/predict_remap_model.py) on hand-made inputs with guard words behind every
output buffer; the golden worlds of the reference through predict.map_reads_to_clusters; predict.map_and_cluster(...,
remap=True) and `annotate --novel-map` end to end against the model route over the files the same run wrote."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from tests import bowtie_text_model as btm
from tests import predict_remap_model as model

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "predict_remap.json")
with open(GOLDEN) as fh:
    WORLDS = json.load(fh)["worlds"]
GUARD = 64
SUFFIX = "_vs_representative_seq_modified_selected_sorted.tsv"


@pytest.fixture(scope="module")
def engine(native_lib):
    from mirge_amd.engine import Engine
    eng = Engine(0)
    yield eng
    eng.close()


def rand_seq(rng, L, n_at=()):
    s = "".join("ACGT"[c] for c in rng.integers(0, 4, L))
    for i in n_at:
        if 0 <= i < L:
            s = s[:i] + "N" + s[i + 1:]
    return s


def tmp_for(engine, n, rows):
    import torch
    need = C.c_uint64()
    assert engine._lib.mrg_predict_remap_temp_bytes(n, rows, C.byref(need)) == 0
    return torch.empty(max(int(need.value), 8), dtype=torch.uint8, device=engine.device), int(need.value)


# --------------------------------------------------------------------------------------------------- the trim kernel
def call_trim_reads(engine, seqs, picked, t5, t3, force_mask=False):
    """mrg_predict_trim_reads on the reads `seqs`, of which picked[r] have no pass-1 alignment; checks the outputs against
    bowtie.trim + pack.pack_reads and the guard words behind them."""
    import torch
    from mirge_amd import bowtie, pack
    L, dev = engine._lib, engine.device
    n = len(seqs)
    W = pack.words_for(max([len(s) for s in seqs] + [1]))
    words, lens, nmask = pack.pack_reads(seqs, W) if n else (np.zeros((W, 0), np.uint64), np.zeros(0, np.uint8), None)
    if nmask is None and force_mask:
        nmask = np.zeros_like(words)
    rng = np.random.default_rng(n + 7 * t5 + t3)
    counts = np.zeros((4, max(n, 1)), dtype=np.uint32)
    for r in range(n):
        if not picked[r]:
            counts[int(rng.integers(0, 4)), r] = int(rng.choice([1, 2, 2 ** 32 - 1]))

    def up(a, view=None):
        a = np.ascontiguousarray(a)
        if a.size == 0:
            a = np.zeros(1, a.dtype)
        return torch.from_numpy(a if view is None else a.view(view)).to(dev)

    def guarded(count, dtype, fill):
        return torch.full((count + GUARD,), fill, dtype=dtype, device=dev)
    d_words, d_lens, d_counts = up(words, np.int64), up(lens), up(counts, np.int32)
    d_nmask = None if nmask is None else up(nmask, np.int64)
    sel, o_words, o_lens = guarded(n, torch.int32, -3), guarded(W * n, torch.int64, -11), guarded(n, torch.uint8, 0xA5)
    o_nmask = guarded(W * n, torch.int64, -13)
    tmp, need = tmp_for(engine, n, 0)
    k = C.c_uint64(77)
    rc = L.mrg_predict_trim_reads(engine._h, d_words.data_ptr(), W, n, d_lens.data_ptr(), None if d_nmask is None else d_nmask.data_ptr(),
                                  n, d_counts.data_ptr(), t5, t3, sel.data_ptr(), o_words.data_ptr(), o_lens.data_ptr(), o_nmask.data_ptr(),
                                  C.byref(k), tmp.data_ptr(), need, engine._stream_ptr())
    assert rc == 0, L.mrg_last_error()
    want_sel = [r for r in range(n) if picked[r]]
    k = int(k.value)
    assert k == len(want_sel)
    # (bowtie.trim slices; a read of t5 + t3 bases or fewer is empty, which the slice alone does not say when len < t3)
    cut = [bowtie.trim(seqs[r], t5, t3) if len(seqs[r]) > t5 + t3 else "" for r in want_sel]
    w2, l2, nm2 = pack.pack_reads(cut, W) if k else (np.zeros((W, 0), np.uint64), np.zeros(0, np.uint8), None)
    assert sel.cpu().numpy()[:k].tolist() == want_sel
    assert np.array_equal(o_words.cpu().numpy()[:W * k].view(np.uint64).reshape(W, k), w2)
    assert np.array_equal(o_lens.cpu().numpy()[:k], l2)
    if d_nmask is not None:
        assert np.array_equal(o_nmask.cpu().numpy()[:W * k].view(np.uint64).reshape(W, k), np.zeros_like(w2) if nm2 is None else nm2)
    for t, valid, fill in ((sel, k, -3), (o_words, W * k, -11), (o_lens, k, 0xA5), (o_nmask, W * k if d_nmask is not None else 0, -13)):
        assert (t.cpu().numpy()[valid:] == fill).all(), "a write behind the valid part of an output buffer"
    return cut


LENGTHS = (0, 3, 4, 5, 16, 31, 32, 33, 36, 63, 64, 65, 68, 255)
TRIMS = ((1, 3), (0, 0), (32, 0), (0, 33))


@pytest.mark.parametrize("trims", TRIMS, ids=lambda t: "%d_%d" % t)
def test_trim_kernel_every_length_with_n_inside_and_in_the_cut_parts(engine, trims):
    rng = np.random.default_rng(31)
    t5, t3 = trims
    seqs = []
    for L in LENGTHS:
        seqs += [rand_seq(rng, L), rand_seq(rng, L, (0,)), rand_seq(rng, L, (L - 1,)), rand_seq(rng, L, (t5, L - t3 - 1)),
                 rand_seq(rng, L, (max(t5 - 1, 0), L - t3, L // 2, 32, 63, 64)), "T" * L]
    picked = [True] * len(seqs)
    cut = call_trim_reads(engine, seqs, picked, t5, t3)
    assert "" in cut and any("N" in c for c in cut) and any(len(c) == 255 - t5 - t3 for c in cut)
    picked = [bool(k % 3) for k in range(len(seqs))]
    call_trim_reads(engine, seqs, picked, t5, t3)
    # the same without an N anywhere: no mask is passed; and with an all-zero mask
    clean = [s.replace("N", "A") for s in seqs]
    call_trim_reads(engine, clean, picked, t5, t3)
    call_trim_reads(engine, clean, picked, t5, t3, force_mask=True)
    short = [s for s in seqs if len(s) <= 64]                 # two words, one word
    call_trim_reads(engine, short, [True] * len(short), t5, t3)
    call_trim_reads(engine, [s for s in short if len(s) <= 32], [True] * sum(len(s) <= 32 for s in short), t5, t3)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 4097])       # 4097: one more than a scan tile
def test_trim_kernel_read_counts_and_none_some_all_picked(engine, n):
    rng = np.random.default_rng(100 + n)
    seqs = [rand_seq(rng, int(rng.integers(0, 70)), (int(rng.integers(0, 90)),)) for _ in range(n)]
    for picked in ([False] * n, [bool(x) for x in rng.integers(0, 2, n)], [True] * n):
        for t5, t3 in ((1, 3), (32, 0)):
            call_trim_reads(engine, seqs, picked, t5, t3)


# ------------------------------------------------------------------------------------------- merge, keys and the sort
def call_rows(engine, numbers, kept, listing1, listing2, sel, expect_error=None):
    """mrg_predict_remap_rows on lists; listing = (offsets, ref, pos, mm).  Returns the rows as tuples after checking the
    guard words behind every output."""
    import torch
    L, dev = engine._lib, engine.device

    def up(x, dt, view=None):
        h = np.array(x if len(x) else [0], dtype=dt)
        return torch.from_numpy(h if view is None else h.view(view)).to(dev)
    d = []
    for off, ref, pos, mm in (listing1, listing2):
        d.append((up(off, np.uint64, np.int64), up(ref, np.int32), up(pos, np.int32), up(mm, np.uint8), len(ref)))
    T = d[0][4] + d[1][4]
    d_num, d_kept, d_sel = up(numbers, np.uint32, np.int32), up(kept, np.uint32, np.int32), up(sel, np.uint32, np.int32)
    outs = [torch.full((T + GUARD,), f, dtype=dt, device=dev) for dt, f in
            ((torch.int32, -3), (torch.int32, -5), (torch.int32, -7), (torch.uint8, 0xA5), (torch.uint8, 0x5A))]
    tmp, need = tmp_for(engine, len(numbers), T)
    ptrs = lambda t: (t[0].data_ptr(), t[4], t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr())
    rc = L.mrg_predict_remap_rows(engine._h, len(numbers), d_num.data_ptr(), len(kept), d_kept.data_ptr(), *ptrs(d[0]), len(sel),
                                  d_sel.data_ptr(), *ptrs(d[1]), *[o.data_ptr() for o in outs], tmp.data_ptr(), need, engine._stream_ptr())
    for o, f in zip(outs, (-3, -5, -7, 0xA5, 0x5A)):
        assert (o.cpu().numpy()[T:] == f).all(), "a write behind the valid part of an output buffer"
    if expect_error is not None:
        assert rc == -1 and expect_error in L.mrg_last_error(), L.mrg_last_error()
        return None
    assert rc == 0, L.mrg_last_error()
    cols = [o.cpu().numpy()[:T] for o in outs]
    return list(zip(cols[0].view(np.uint32).tolist(), cols[1].view(np.uint32).tolist(), cols[2].view(np.uint32).tolist(),
                    cols[3].tolist(), cols[4].tolist()))


def listings(seed, n, K, rows=None, big=False, pass1=True, pass2=True):
    """Hand-made listings: per read 0..3 pass-1 rows; the reads without one go to pass 2 with 0..3 rows; clusters repeat
    inside a read's rows, so (cluster, read) pairs come more than once."""
    rng = np.random.default_rng(seed)
    hi = 2 ** 32 if big else 1200
    numbers = sorted(set([1, 9, 10, 99, 100] + [int(x) for x in rng.integers(1, hi - 1, 2 * n)]))[:n - 1] + [hi - 1]
    numbers = [numbers[int(j)] for j in rng.permutation(len(numbers))]
    n = len(numbers)
    kept = sorted(set([0, 8, 9, 98, 99, hi - 2] + [int(x) for x in rng.integers(0, hi - 1, 2 * K)]))
    kept = kept[:K - 1] + [hi - 2] if K > 1 else kept[:K]
    K = len(kept)
    c1 = [int(x) if pass1 else 0 for x in rng.choice([0, 0, 1, 2, 3], n)]
    if rows is not None:
        c1[-1] = max(c1[-1], 1)
    top = numbers.index(hi - 1)                                 # the largest read number owns a row on the largest cluster number
    if pass1:
        c1[top] = max(c1[top], 1)
    sel = [r for r in range(n) if c1[r] == 0]
    c2 = [int(x) if pass2 else 0 for x in rng.choice([0, 1, 2, 3], len(sel))]
    if rows is not None:                                        # exactly `rows` rows: the last read takes the rest
        short = rows - sum(c1) - sum(c2)
        assert short >= 0
        c1[-1] += short

    def listing(counts):
        off = [0]
        for c in counts:
            off.append(off[-1] + c)
        t = off[-1]
        few = max(1, min(K, 3))
        ref = [int(x) for x in np.where(rng.random(t) < 0.5, rng.integers(0, few, t), rng.integers(0, K, t))]
        return off, ref, [int(x) for x in rng.integers(0, 14, t)], [int(x) for x in rng.integers(0, 3, t)]
    l1 = listing(c1)
    if pass1:
        l1[1][l1[0][top]] = K - 1
    return numbers, kept, l1, listing(c2), sel


def check_rows(engine, numbers, kept, l1, l2, sel):
    want = model.sort_rows(model.merge(l1, l2, sel), numbers, [k + 1 for k in kept])
    got = call_rows(engine, numbers, kept, l1, l2, sel)
    assert got == want
    return want


@pytest.mark.parametrize("case", ["both", "no_pass1", "no_pass2", "neither", "big_numbers"])
def test_rows_against_the_model(engine, case):
    args = listings(5, 90, 23, big=case == "big_numbers", pass1=case not in ("no_pass1", "neither"), pass2=case not in ("no_pass2", "neither"))
    want = check_rows(engine, *args)
    if case in ("both", "big_numbers"):
        pairs = [w[:2] for w in want]
        assert len(set(pairs)) < len(pairs) and {0, 1} == {w[4] for w in want}
        by_digits = [(str(args[1][w[1]] + 1) + "_", str(args[0][w[0]]) + "_") for w in want]
        assert by_digits == sorted(by_digits) and by_digits != sorted(by_digits, key=lambda p: (int(p[0][:-1]), int(p[1][:-1])))
    if case == "big_numbers":
        assert 2 ** 32 - 1 in [args[0][w[0]] for w in want] and 2 ** 32 - 2 in [args[1][w[1]] for w in want]
    if case == "neither":
        assert want == []


def test_rows_4097_and_one_read_one_cluster(engine):
    numbers, kept, l1, l2, sel = listings(6, 1500, 40, rows=4097)
    assert len(l1[1]) + len(l2[1]) == 4097
    check_rows(engine, numbers, kept, l1, l2, sel)
    check_rows(engine, [4], [6], ([0, 3], [0, 0, 0], [5, 0, 2], [0, 1, 2]), ([0], [], [], []), [])
    check_rows(engine, [4, 2 ** 32 - 1], [2 ** 32 - 2], ([0, 0, 0], [], [], []), ([0, 2], [0, 0], [1, 0], [1, 1]), [1])


def test_rows_inconsistent_arrays_are_errors_and_write_nothing_out_of_bounds(engine):
    numbers, kept, l1, l2, sel = listings(8, 200, 30)
    check_rows(engine, numbers, kept, l1, l2, sel)
    off = list(l1[0])
    off[100] = off[-1] + 1000
    call_rows(engine, numbers, kept, (off,) + l1[1:], l2, sel, expect_error=b"offsets")
    off = list(l1[0])
    off[0] = 2
    call_rows(engine, numbers, kept, (off,) + l1[1:], l2, sel, expect_error=b"offsets")
    off = [x + (1 if k == len(l2[0]) - 1 else 0) for k, x in enumerate(l2[0])]
    call_rows(engine, numbers, kept, l1, (off,) + l2[1:], sel, expect_error=b"offsets")
    ref = list(l1[1])
    ref[len(ref) // 2] = len(kept)
    call_rows(engine, numbers, kept, (l1[0], ref) + l1[2:], l2, sel, expect_error=b"clusters")
    pos = list(l2[2])
    pos[0] = -1
    call_rows(engine, numbers, kept, l1, l2[:2] + (pos, l2[3]), sel, expect_error=b"clusters")
    owner = [r for r in range(len(sel)) if l2[0][r + 1] > l2[0][r]][0]
    bad_sel = list(sel)
    bad_sel[owner] = len(numbers)
    call_rows(engine, numbers, kept, l1, l2, bad_sel, expect_error=b"pass-2 read")
    L = engine._lib
    assert L.mrg_predict_remap_rows(engine._h, 5, None, 3, None, None, 4, None, None, None, 0, None, None, 0, None, None, None, None, None,
                                    None, None, None, None, 0, None) < 0 and b"null" in L.mrg_last_error()


# ------------------------------------------------------------------------------------------------------- end to end
def world_inputs(engine, w, stem):
    from mirge_amd import pack
    from mirge_amd.engine import ReadSet
    names, seqs = model.parse_fasta(w["reads_fa"])
    _, _, kept, soff, orig = model.cluster_arrays(w["clusters_fa"])
    with open(stem + "_vs_genome_sorted_clusters_trimmed_orig.fa", "w") as fh:
        fh.write(w["clusters_fa"])
    rs = ReadSet(*pack.pack_reads(seqs), device=engine.device)
    trim = dict(kept=np.array(kept, np.uint32), kept_seq_off=np.array(soff, np.uint64), kept_orig=orig, n_retained=len(kept))
    numbers = np.array([model.read_number(n) for n in names], np.uint32)
    counts = np.array([int(n.split("_")[-1]) for n in names], np.uint32)
    return rs, numbers, counts, trim, names


@pytest.mark.parametrize("w", WORLDS, ids=lambda w: w["name"])
def test_golden_worlds_through_map_reads_to_clusters(engine, tmp_path, w):
    from mirge_amd import predict
    stem = str(tmp_path / "unmapped_mirna_smp")
    rs, numbers, counts, trim, names = world_inputs(engine, w, stem)
    libs = dict(engine.libs)
    got = predict.map_reads_to_clusters(engine, rs, numbers, counts, trim, w["seed_length"], stem, names)
    assert open(stem + SUFFIX).read() == w["table"]
    again = predict.map_reads_to_clusters(engine, rs, None, counts, trim, w["seed_length"], stem, names)   # (numbers from the names)
    assert open(stem + SUFFIX).read() == w["table"]
    assert engine.libs == libs
    lines = w["table"].splitlines()
    assert got["n_rows"] == again["n_rows"] == len(lines) == len(got["rows"][0])
    assert got["aligned1"] + got["aligned2"] + got["unaligned"] == len(names)
    assert got["aligned1"] + got["aligned2"] == len(set(ln.split("\t")[0] for ln in lines))
    assert got["aligned2"] == len(set(ln.split("\t")[0] for ln in lines if len(ln.split("\t")[12]) != len(ln.split("\t")[2])))
    assert [names[r] for r in got["rows"][0]] == [ln.split("\t")[0] for ln in lines]
    assert "device" not in got and got["rows"][3].dtype == np.uint8


def test_no_retained_cluster_writes_nothing(engine, tmp_path):
    from mirge_amd import predict
    stem = str(tmp_path / "unmapped_mirna_smp")
    rs, numbers, counts, _, names = world_inputs(engine, WORLDS[0], stem)
    os.remove(stem + "_vs_genome_sorted_clusters_trimmed_orig.fa")
    trim = dict(kept=np.zeros(0, np.uint32), kept_seq_off=np.zeros(1, np.uint64), kept_orig=b"", n_retained=0)
    got = predict.map_reads_to_clusters(engine, rs, numbers, counts, trim, 25, stem, names)
    assert os.listdir(str(tmp_path)) == [] and got["n_rows"] == got["aligned1"] == got["aligned2"] == got["unaligned"] == 0


def model_table_of(sub, base, seed_length):
    """bowtie_text_model twice over the files a run wrote, then the model."""
    reads_fa = open(os.path.join(sub, base + ".fa")).read()
    clusters_fa = open(os.path.join(sub, base + "_vs_genome_sorted_clusters_trimmed_orig.fa")).read()
    parts = [model.parse_fasta(clusters_fa)]
    sam1, _ = btm.run(model.pass1_argv(seed_length) + ["ix", "reads.fa"], parts, reads_fa)
    sam2, _ = btm.run(model.PASS2_ARGV + ["ix", "left.fa"], parts, model.unaligned_fasta(sam1, reads_fa))
    return model.table_from_sam(sam1, sam2, reads_fa, clusters_fa)


def twin_loci(texts):
    """chr2 carries one 30-mer at two loci: the reads cut there sit in two clusters."""
    texts[1] = texts[1][:7500] + texts[1][7000:7030] + texts[1][7530:]


def extra_reads(texts):
    flip = lambda s: "ACGT"[("ACGT".index(s[0]) + 1) % 4] + s[1:]
    out = [texts[1][7000:7000 + L] for L in (18, 20, 22)]                       # two clusters each
    out += [flip(texts[1][500:521]), flip(texts[1][7001:7022]), texts[1][500:518] + "GAT"]   # aligned in pass 2 only
    return out


def test_map_and_cluster_with_remap_equals_the_model_route(engine, oracle_lib, tmp_path):
    from mirge_amd import predict
    from mirge_amd.index import FmIndex
    from tests.test_gpu_predict_trim import REPEATS_TSV, SUFFIXES, piles
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
    trimmed, mapped = tmp_path / "trimmed", tmp_path / "mapped"
    trimmed.mkdir()
    mapped.mkdir()
    cl0 = predict.map_and_cluster(engine, str(fa), genome, 3, 25, 14, str(trimmed / "unmapped_mirna_s1"), trim=(str(tmp_path / "rep.tsv"), 24))
    libs = dict(engine.libs)
    cl = predict.map_and_cluster(engine, str(fa), genome, 3, 25, 14, str(mapped / "unmapped_mirna_s1"), trim=(str(tmp_path / "rep.tsv"), 24),
                                 remap=True)
    assert engine.libs == libs
    base = "unmapped_mirna_s1"
    five = [base + "_vs_genome_sorted.sam", base + "_vs_genome_sorted_clusters.tsv"] + [base + "_vs_genome_sorted_clusters" + s for s in SUFFIXES]
    assert sorted(os.listdir(str(trimmed))) == sorted(five) and sorted(os.listdir(str(mapped))) == sorted(five + [base + SUFFIX])
    for fn in five:
        assert (trimmed / fn).read_bytes() == (mapped / fn).read_bytes(), fn
    assert sorted(set(cl) - set(cl0)) == ["remap"] and "device" not in cl["remap"]
    (mapped / (base + ".fa")).write_text(fa.read_text())
    want, rows = model_table_of(str(mapped), base, 25)
    assert (mapped / (base + SUFFIX)).read_text() == want
    by_read = {}
    for r, c, _, _, p in rows:
        by_read.setdefault(r, set()).add(c)
    assert any(p == 1 for _, _, _, _, p in rows) and any(len(v) > 1 for v in by_read.values()) and len(rows) > 50
    assert cl["remap"]["n_rows"] == len(rows) and cl["remap"]["aligned2"] == len({r for r, _, _, _, p in rows if p == 1})
    # the shell's way to the same six files
    shell = tmp_path / "shell"
    shell.mkdir()
    assert predict.main(["clusters", genome, str(fa), "-o", str(shell / base), "--trim", "--repeats", str(tmp_path / "rep.tsv"),
                         "-clc", "24", "--remap"]) == 0
    os.remove(str(mapped / (base + ".fa")))
    assert sorted(os.listdir(str(shell))) == sorted(os.listdir(str(mapped)))
    assert (shell / (base + SUFFIX)).read_bytes() == (mapped / (base + SUFFIX)).read_bytes()


def test_cli_novel_map_adds_one_file_per_sample_and_leaves_the_others_alone(tmp_path_factory, native_lib, oracle_lib, tmp_path):
    from mirge_amd import cli
    from mirge_amd.index import FmIndex
    from tests import util
    from tests.test_gpu_predict_trim import REPEATS_TSV, piles
    from tests.test_gpu_predict_trim import rand_seq as plain_seq
    w = util.World(n_fixed=600, n_var=150)
    root = str(tmp_path_factory.mktemp("remap_libs") / "libs")
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
    before = annotate(tmp_path / "trim", "--novel-trim", "-clc", "24", "-sl", "18")
    after = annotate(tmp_path / "map", "--novel-map", "-clc", "24", "-sl", "18")
    assert sorted(os.listdir(before)) == sorted(os.listdir(after))
    for stem in ("left", "right"):
        sub = "unmapped_mirna_%s_tmp" % stem
        base = "unmapped_mirna_" + stem
        old = sorted(os.listdir(os.path.join(before, sub)))
        assert len(old) == 7 and sorted(os.listdir(os.path.join(after, sub))) == sorted(old + [base + SUFFIX])
        for fn in old:
            assert open(os.path.join(before, sub, fn), "rb").read() == open(os.path.join(after, sub, fn), "rb").read(), fn
        want, rows = model_table_of(os.path.join(after, sub), base, 18)
        assert open(os.path.join(after, sub, base + SUFFIX)).read() == want
        assert any(r[4] == 1 for r in rows) and any(r[4] == 0 for r in rows)
