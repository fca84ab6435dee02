"""Predict mode's preliminary trim on the GPU (-m gpu): mrg_predict_trim on hand-made device arrays against the sequential
model (tests/predict_trim_model.py) with guard bytes behind every output buffer, the golden worlds of the reference through
Engine.predict_trim and the native writer, predict.map_and_cluster(..., trim=...) and `annotate --novel-trim` end to end
against the model over the cluster table the same run wrote."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest

from tests import predict_trim_model as model

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "predict_trim.json")
with open(GOLDEN) as fh:
    WORLDS = json.load(fh)["worlds"]
SUFFIXES = ("_trimmed.tsv", "_trimmed.fa", "_trimmed_orig.fa")
GUARD = 64
BIG = 2 ** 31 - 1


@pytest.fixture(scope="module")
def engine(native_lib):
    from mirge_amd.engine import Engine
    eng = Engine(0)
    yield eng
    eng.close()


def call_trim(engine, a, rep_off, rep_start, rep_end, cutoff, expect_error=None):
    """mrg_predict_trim on the lists of `a` (entry, strand, start, end, seq_off, seq str) -> the outputs as lists / str, after
    checking that nothing behind or between the valid parts of the output buffers was written."""
    import torch
    L, dev = engine._lib, engine.device
    K, total = len(a["entry"]), len(a["seq"])

    def up(x, dt, view=None):
        h = np.array(x if len(x) else [0], dtype=dt)          # (a copy: torch wants writable memory)
        return torch.from_numpy(h if view is None else h.view(view)).to(dev)

    def guarded(count, dtype, fill):
        return torch.full((count + GUARD,), fill, dtype=dtype, device=dev)
    entry, start, end = (up(a[k], np.uint32, np.int32) for k in ("entry", "start", "end"))
    strand = up(a["strand"], np.uint8)
    seq_off = up(a["seq_off"], np.uint64, np.int64)
    seq = up(np.frombuffer(a["seq"].encode(), dtype=np.uint8), np.uint8)
    r_off, r_start, r_end = (up(x, np.uint32, np.int32) for x in (rep_off, rep_start, rep_end))
    flag, rep, orig = guarded(K, torch.uint8, 0xA5), guarded(K, torch.int32, -77), guarded(total, torch.uint8, 0x5A)
    kept, kept_off, kept_orig = guarded(K, torch.int32, -5), guarded(K + 1, torch.int64, -9), guarded(total, torch.uint8, 0x5A)
    need = C.c_uint64()
    assert L.mrg_predict_trim_temp_bytes(K, C.byref(need)) == 0
    tmp = torch.empty(int(need.value), dtype=torch.uint8, device=dev)
    n_kept, kept_len = C.c_uint64(), C.c_uint64()
    rc = L.mrg_predict_trim(engine._h, K, entry.data_ptr(), strand.data_ptr(), start.data_ptr(), end.data_ptr(), seq_off.data_ptr(),
                            seq.data_ptr(), total, len(rep_off) - 1, r_off.data_ptr(), r_start.data_ptr(), r_end.data_ptr(),
                            len(rep_start), int(cutoff), flag.data_ptr(), rep.data_ptr(), orig.data_ptr(), kept.data_ptr(),
                            kept_off.data_ptr(), kept_orig.data_ptr(), C.byref(n_kept), C.byref(kept_len), tmp.data_ptr(),
                            need.value, engine._stream_ptr())
    if expect_error is not None:
        assert rc < 0 and expect_error in L.mrg_last_error()
        for t, n, fill in ((flag, K, 0xA5), (rep, K, -77), (orig, total, 0x5A), (kept, K, -5), (kept_off, K + 1, -9), (kept_orig, total, 0x5A)):
            assert (t.cpu().numpy()[n:] == fill).all()
        return None
    assert rc == 0, L.mrg_last_error()
    nk, kl = int(n_kept.value), int(kept_len.value)
    for t, n, fill in ((flag, K, 0xA5), (rep, K, -77), (orig, total, 0x5A), (kept, nk, -5), (kept_off, nk + 1, -9), (kept_orig, kl, 0x5A)):
        assert (t.cpu().numpy()[n:] == fill).all(), "a write behind the valid part of an output buffer"
    return dict(flag=flag.cpu().numpy()[:K].tolist(), rep=rep.cpu().numpy()[:K].tolist(), orig=orig.cpu().numpy()[:total].tobytes().decode(),
                kept=kept.cpu().numpy()[:nk].tolist(), kept_seq_off=kept_off.cpu().numpy()[:nk + 1].tolist(),
                kept_orig=kept_orig.cpu().numpy()[:kl].tobytes().decode())


def check(engine, a, rep, cutoff):
    rep_off, rep_start, rep_end = rep
    want = model.trim(a["entry"], a["strand"], a["start"], a["end"], a["seq_off"], a["seq"], rep_off, rep_start, rep_end, cutoff)
    got = call_trim(engine, a, rep_off, rep_start, rep_end, cutoff)
    for k in ("flag", "rep", "orig", "kept", "kept_seq_off", "kept_orig"):
        assert got[k] == want[k], k
    return want


def arrays(clusters):
    """clusters: (entry, strand, start, sequence) -> the cluster arrays as lists."""
    seq_off = [0]
    for c in clusters:
        seq_off.append(seq_off[-1] + len(c[3]))
    return dict(entry=[c[0] for c in clusters], strand=[c[1] for c in clusters], start=[c[2] for c in clusters],
                end=[c[2] + len(c[3]) - 1 for c in clusters], seq_off=seq_off, seq="".join(c[3] for c in clusters))


def rand_seq(rng, L, p_n=0.0):
    s = "".join("ACGT"[c] for c in rng.integers(0, 4, L))
    if L and rng.random() < p_n:
        i = int(rng.integers(0, L))
        s = s[:i] + "N" + s[i + 1:]
    return s


def table_of(counts, rng, span=20000):
    """A repeat table with counts[e] elements on entry e: starts with repeats among them, ends before, at and after them."""
    rep_off, start, end = [0], [], []
    for n in counts:
        s = sorted(int(x) for x in rng.integers(1, span, n))
        if n >= 3:
            s[1] = s[0]                                   # equal starts
        start += s
        end += [x + int(rng.integers(-3, 80)) for x in s]
        rep_off.append(len(start))
    return rep_off, start, [max(e, 0) for e in end]


@functools.lru_cache(maxsize=None)
def random_world(K):
    rng = np.random.default_rng(900 + K)
    rep = table_of([40, 0, 300], rng)                     # an entry without a table between two that have one
    clusters = []
    for _ in range(K):
        e = int(rng.integers(0, 3))
        lo, hi = rep[0][e], rep[0][e + 1]
        if hi > lo and rng.random() < 0.6:                # near an element, often right on its start
            start = max(1, rep[1][int(rng.integers(lo, hi))] + int(rng.choice([0, 0, 1, -1, 7, -20, 35])))
        else:
            start = int(rng.integers(1, 21000))
        L = int(rng.choice([1, 2, 5, 6, 7, 16, 22, 29, 30, 31, 40]))
        seq = rand_seq(rng, L, 0.1)
        kind = rng.random()
        if kind < 0.08:
            seq = seq[:max(L - 6, 0)] + "A" * min(L, 6)
        elif kind < 0.16:
            seq = "T" * min(L, 6) + seq[min(L, 6):]
        clusters.append((e, int(rng.integers(0, 2)), start, seq))
    return arrays(clusters), rep


@pytest.mark.parametrize("K", [0, 1, 63, 64, 65, 4097])     # 4097: one more than a scan tile
def test_cluster_counts_around_the_wave_and_the_scan_tile(engine, K):
    a, rep = random_world(K)
    want = check(engine, a, rep, 30)
    if K >= 63:
        assert 0 < sum(want["flag"]) < K and any(r >= 0 for r in want["rep"]) and 1 in a["strand"] and 0 in a["strand"]
    check(engine, a, rep, 0 if K < 100 else 6)


def run_cases():
    mid = "CGCGTACGTACG"
    out = []
    for k in (5, 6, 7):
        out += [mid + "A" * k, "T" * k + mid, "A" * k + mid, mid + "T" * k, "G" + "A" * k, mid[:6] + "A" * k + "C", "A" * k, "T" * k]
    return out + ["A" * 30, "T" * 30, "A", "T", "N", "NAAAAAA", "TTTTTTN"]


def test_sequences_across_the_64_and_256_byte_boundaries_of_the_buffer(engine):
    """Every end-run case on both strands, once ending on a multiple of 64 / 256 bytes of the concatenated buffer and once
    beginning there; fillers of 1 nt and of lengths that straddle the boundaries in between."""
    rng = np.random.default_rng(12)
    clusters, off, ends_on, begins_on = [], 0, set(), set()

    def put(strand, seq):
        nonlocal off
        clusters.append((0, strand, 1000 + 50 * len(clusters), seq))
        if (off + len(seq)) % 64 == 0:
            ends_on.add(256 if (off + len(seq)) % 256 == 0 else 64)
        if off % 64 == 0 and off:
            begins_on.add(256 if off % 256 == 0 else 64)
        off += len(seq)
    for i, case in enumerate(run_cases() * 2):
        strand = (i // len(run_cases())) % 2
        B = 256 if i % 3 == 0 else 64
        fill = (-(off + len(case))) % B                   # the case ends on a multiple of B ...
        while fill:
            step = min(fill, int(rng.choice([1, 1, 3, 40])))
            put(int(rng.integers(0, 2)), rand_seq(rng, step, 0.2))
            fill -= step
        put(strand, case)
        put(strand, case)                                 # ... and its twin begins there
        put(int(rng.integers(0, 2)), rand_seq(rng, int(rng.choice([63, 65, 130])), 0.2))   # straddles the next boundary
    assert ends_on == begins_on == {64, 256}
    a = arrays(clusters)
    want = check(engine, a, ([0, 0], [], []), 30)
    assert 0 in want["flag"] and 1 in want["flag"]
    check(engine, a, ([0, 0], [], []), 300)               # the cutoff out of the way: only the ends decide


def test_tables_of_0_1_2_3_and_1000_elements(engine):
    rng = np.random.default_rng(13)
    counts = [0, 1, 2, 3, 1000]
    rep = table_of(counts, rng)
    clusters = []
    for e, n in enumerate(counts):
        lo, hi = rep[0][e], rep[0][e + 1]
        starts = [1, 19999, 25000] + [int(x) for x in rng.integers(1, 21000, 30)]
        for x in range(lo, min(hi, lo + 40)):             # on an element's start, one before, one after, inside, behind its end
            starts += [rep[1][x], max(1, rep[1][x] - 1), rep[1][x] + 1, max(1, rep[1][x] - 19), rep[2][x] + 1]
        if n:
            starts += [max(1, min(rep[1][lo:hi]) - 30), max(rep[1][lo:hi]) + 30]   # before all starts, after all starts
        clusters += [(e, int(rng.integers(0, 2)), s, rand_seq(rng, int(rng.choice([16, 20, 25])))) for s in starts]
    want = check(engine, arrays(clusters), rep, 30)
    for e in range(1, 5):
        hit = [want["rep"][i] for i, c in enumerate(clusters) if c[0] == e and want["rep"][i] >= 0]
        assert hit and all(rep[0][e] <= x < rep[0][e + 1] for x in hit)
    assert all(want["flag"][i] == 1 for i, c in enumerate(clusters) if c[0] == 0)


def test_ties_equal_starts_and_elements_that_cover_nothing(engine):
    # entry 0: three elements at distance 50 of 1050, two sharing a start; entry 1: 550 and 650 at equal distance of 600;
    # entry 2: end < start; entry 3: a run of five equal starts in front of the cluster
    rep = ([0, 3, 6, 8, 14], [1000, 1000, 1100, 500, 550, 650, 1000, 1200, 90, 100, 100, 100, 100, 100],
           [1060, 1005, 1100, 520, 640, 660, 900, 1199, 95, 101, 102, 300, 103, 104])
    clusters = [(0, 0, 1050, "ACGTACGTACGTACGTACGT"), (0, 1, 1050, "ACGTACGTACGTACGTACGT"), (1, 0, 600, "ACGTACGTACGTACGTACGT"),
                (1, 0, 601, "ACGTACGTACGTACGTACGT"), (1, 0, 599, "ACGTACGTACGTACGTACGT"), (2, 0, 950, "ACGTACGTACGTACGTACGT"),
                (2, 0, 1190, "ACGTACGTACGTACGTACGT"), (3, 0, 150, "ACGTACGTACGTACGTACGT"), (3, 0, 100, "ACGTACGTACGTACGTACGT"),
                (3, 0, 96, "ACGTACGTACGTACGTACGT")]
    want = check(engine, arrays(clusters), rep, 30)
    assert want["rep"][0] == 0 and want["flag"][0] == 0   # the lower index of the two at 1000, not the element at 1100
    assert want["rep"][2] == 4                            # 550 before 650 at equal distance
    assert want["flag"][5] == 1 and want["flag"][6] == 1  # nothing is covered by an element with end < start
    assert want["rep"][7] == -1                           # of the five at 100 the first two are looked at: they end at 101, 102
    assert want["rep"][8] == 9


def test_positions_near_2_to_the_31_and_beyond(engine):
    rng = np.random.default_rng(14)
    rep = ([0, 6], [5, BIG - 40, BIG - 1, BIG, 2 ** 32 - 60, 2 ** 32 - 2], [9, BIG - 30, BIG - 1, BIG + 10, 2 ** 32 - 50, 2 ** 32 - 1])
    starts = [BIG - 60, BIG - 45, BIG - 35, BIG - 20, BIG - 2, BIG - 1, BIG, 1, 2 ** 30, (BIG + 5 + 2 ** 32 - 60) // 2]
    clusters = [(0, int(rng.integers(0, 2)), s, rand_seq(rng, L)) for s in starts for L in (1, 16, 30)]
    want = check(engine, arrays(clusters), rep, 30)
    assert 0 in want["flag"] and 1 in want["flag"] and {1, 2, 3} <= set(want["rep"])


def test_inconsistent_inputs_are_errors_and_write_nothing_out_of_bounds(engine):
    rng = np.random.default_rng(15)
    rep = table_of([5, 5], rng)
    a = arrays([(int(rng.integers(0, 2)), 0, int(rng.integers(1, 20000)), rand_seq(rng, 20)) for _ in range(70)])
    check(engine, a, rep, 30)
    call_trim(engine, dict(a, entry=a["entry"][:-1] + [2]), *rep, 30, expect_error=b"entry")
    bad_off = list(a["seq_off"])
    bad_off[40] = bad_off[-1] + 1000
    call_trim(engine, dict(a, seq_off=bad_off), *rep, 30, expect_error=b"d_seq_off")
    call_trim(engine, a, [0, 5, 11], rep[1], rep[2], 30, expect_error=b"d_rep_off")
    L = engine._lib
    out = C.c_uint64()
    assert L.mrg_predict_trim(engine._h, 3, None, None, None, None, None, None, 0, 0, None, None, None, 0, 30, None, None, None, None,
                              None, None, C.byref(out), C.byref(out), None, 0, None) < 0 and b"null" in L.mrg_last_error()


# ------------------------------------------------------------------------------------- the golden worlds, the Python route
def genome_of(entries):
    from mirge_amd.index import FmIndex
    return [FmIndex.build(list(entries), ["ACGTTGCAAC" * 3] * len(entries))]


@pytest.mark.parametrize("w", WORLDS, ids=lambda w: w["name"])
def test_golden_worlds_through_the_engine_and_the_writer(engine, tmp_path, w):
    from mirge_amd import predict
    entries, rows, a, names, count_sum, member_off, members, rep_tsv = model.world_inputs(w["table"], w["elements"])
    (tmp_path / "rep.tsv").write_text(rep_tsv)
    repeats = predict.load_repeats(str(tmp_path / "rep.tsv"), genome_of(entries))
    cl = dict(a, seq=a["seq"].encode(), count_sum=count_sum, member_off=member_off, members=members)
    stem = str(tmp_path / "smp_a_b_c")                     # (sample_name drops the last three `_` fields of `<stem>_vs_genome_sorted.sam`)
    t = predict.trim_clusters(engine, cl, repeats, w["cutoff"], stem, names)
    got = [open(stem + "_vs_genome_sorted_clusters" + sfx).read() for sfx in SUFFIXES]
    sample = predict.sample_name(stem + "_vs_genome_sorted.sam")
    want = list(model.files(w["table"], w["elements"], w["cutoff"])) if w["ties"] else [w["trimmed_tsv"], w["trimmed_fa"], w["trimmed_orig_fa"]]
    assert got == [x.replace("smp:miRCluster_", sample + ":miRCluster_") for x in want]
    assert t["n_retained"] == want[1].count(">") == len(t["kept"]) and t["flag"].dtype == np.uint8 and t["rep"].dtype == np.int32


JITTER = {500: 0, 530: 4, 4000: 1, 4010: 1, 9000: 0, 12000: 6}   # tight piles stay below the length cutoff, loose ones pass it


def piles(rng, texts, n):
    """Reads of 18-22 nt cut around a few loci of every entry, both strands."""
    comp = str.maketrans("ACGT", "TGCA")
    reads = []
    for _ in range(n):
        e = int(rng.integers(0, len(texts)))
        locus = int(rng.choice(list(JITTER)))
        at = locus + int(rng.integers(-JITTER[locus], JITTER[locus] + 1))
        q = texts[e][at:at + int(rng.integers(18, 23))]
        reads.append(q[::-1].translate(comp) if rng.random() < 0.4 else q)
    return list(dict.fromkeys(reads))


REPEATS_TSV = ("chr1\t480\t560\tAlu_1\nchr1\t4030\t4031\tdot\nchr1\t8990\t9100\tL1_a\nchr1\t300\t20000\tgiant\nchr1\t12100\t12000\tback\n"
               "chr2\t3990\t4005\tMIR_2\nchrNot\t1\t99999\tnowhere\nscaffold_9\t1\t20000\tunseen\n")


def model_files_of(table_path, cutoff):
    elements = {}
    for line in REPEATS_TSV.splitlines():
        ch, s, e, nm = line.split("\t")
        elements.setdefault(ch, []).append((int(s), int(e), nm))
    return list(model.files(open(table_path).read(), elements, cutoff))


def test_map_and_cluster_with_trim_equals_the_model_over_its_own_table(engine, tmp_path):
    from mirge_amd import predict
    from mirge_amd.index import FmIndex
    rng = np.random.default_rng(48)
    names = ["chr1", "chr2", "scaffold_9"]
    texts = [rand_seq(rng, 20000) for _ in names]
    # poly-A / poly-T loci, so that the end tests decide some clusters on both strands
    texts[0] = texts[0][:12000] + "CGCGTACGTACG" + "A" * 7 + "G" + "T" * 7 + "CGCATGCATGCA" + texts[0][12039:]
    genome = str(tmp_path / "syn_genome")
    FmIndex.build(names, texts).save(genome + ".mrgfm")
    reads = piles(rng, texts, 500)
    fa = tmp_path / "unmapped_mirna_s1.fa"
    fa.write_text("".join(">mir%d_%d\n%s\n" % (k + 1, 2 + k % 5, r) for k, r in enumerate(reads)))
    (tmp_path / "rep.tsv").write_text(REPEATS_TSV)
    plain, trimmed = tmp_path / "plain", tmp_path / "trimmed"
    plain.mkdir()
    trimmed.mkdir()
    cl0 = predict.map_and_cluster(engine, str(fa), genome, 3, 25, 14, str(plain / "unmapped_mirna_s1"))
    cl = predict.map_and_cluster(engine, str(fa), genome, 3, 25, 14, str(trimmed / "unmapped_mirna_s1"),
                                 trim=(str(tmp_path / "rep.tsv"), 24))
    base = "unmapped_mirna_s1_vs_genome_sorted"
    assert sorted(os.listdir(str(plain))) == [base + ".sam", base + "_clusters.tsv"]
    assert sorted(os.listdir(str(trimmed))) == sorted([base + ".sam", base + "_clusters.tsv"] + [base + "_clusters" + s for s in SUFFIXES])
    for fn in os.listdir(str(plain)):                     # the two files of the route without trim are what they were
        assert (plain / fn).read_bytes() == (trimmed / fn).read_bytes(), fn
    assert "trim" not in cl0 and "device" not in cl0 and "device" not in cl and sorted(set(cl) - set(cl0)) == ["trim"]
    want = model_files_of(str(trimmed / (base + "_clusters.tsv")), 24)
    got = [(trimmed / (base + "_clusters" + s)).read_text() for s in SUFFIXES]
    assert got == want
    flags = [r[2] for r in model.parse_table(got[0])[1]]
    names_hit = {r[3] for r in model.parse_table(got[0])[1]}
    assert len(flags) > 8 and "0" in flags and "1" in flags and {"Alu_1", "*"} <= names_hit and "unseen" not in names_hit
    assert cl["trim"]["n_retained"] == flags.count("1")
    # the shell's way to the same five files
    shell = tmp_path / "shell"
    shell.mkdir()
    assert predict.main(["clusters", genome, str(fa), "-o", str(shell / "unmapped_mirna_s1"), "--trim", "--repeats",
                         str(tmp_path / "rep.tsv"), "-clc", "24"]) == 0
    assert sorted(os.listdir(str(shell))) == sorted(os.listdir(str(trimmed)))
    for fn in os.listdir(str(trimmed)):
        assert (shell / fn).read_bytes() == (trimmed / fn).read_bytes(), fn
    # the same table without a repeat file: every chromosome passes the repeat test
    none = tmp_path / "none"
    none.mkdir()
    predict.map_and_cluster(engine, str(fa), genome, 3, 25, 14, str(none / "unmapped_mirna_s1"), sam=False, trim=(None, 24))
    rows = model.parse_table((none / (base + "_clusters_trimmed.tsv")).read_text())[1]
    assert {r[3] for r in rows} == {"*"} and [r[2] for r in rows].count("1") > flags.count("1")


# ------------------------------------------------------------------------------------------------------- command line
def test_cli_novel_trim_adds_three_files_and_leaves_the_others_alone(tmp_path_factory, native_lib, tmp_path):
    from mirge_amd import cli
    from mirge_amd.index import FmIndex
    from tests import util
    w = util.World(n_fixed=600, n_var=150)
    root = str(tmp_path_factory.mktemp("trim_libs") / "libs")
    w.libs.write_layout(root, species="syn", db="miRBase")
    rng = np.random.default_rng(47)
    names = ["chr1", "chr2", "scaffold_9"]
    texts = [rand_seq(rng, 20000) for _ in names]
    novel = piles(rng, texts, 400)
    fastqs = []
    for i, name in enumerate(("left.fastq", "right.fastq")):
        reads = list(w.reads[i::2][:300]) + [r for r in novel for _ in range(int(rng.choice([0, 1, 2, 3, 5])))]
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
    before = annotate(tmp_path / "clusters", "--novel-clusters")
    after = annotate(tmp_path / "trim", "--novel-trim", "-clc", "24")
    assert sorted(os.listdir(before)) == sorted(os.listdir(after))
    for stem in ("left", "right"):
        sub = "unmapped_mirna_%s_tmp" % stem
        base = "unmapped_mirna_" + stem
        four = [base + ".fa", base + "_raw.fa", base + "_vs_genome_sorted.sam", base + "_vs_genome_sorted_clusters.tsv"]
        three = [base + "_vs_genome_sorted_clusters" + s for s in SUFFIXES]
        assert sorted(os.listdir(os.path.join(before, sub))) == sorted(four)
        assert sorted(os.listdir(os.path.join(after, sub))) == sorted(four + three)
        for fn in four:
            assert open(os.path.join(before, sub, fn), "rb").read() == open(os.path.join(after, sub, fn), "rb").read(), fn
        want = model_files_of(os.path.join(after, sub, four[3]), 24)
        assert [open(os.path.join(after, sub, fn)).read() for fn in three] == want
        flags = [r[2] for r in model.parse_table(want[0])[1]]
        assert "0" in flags and "1" in flags and len(flags) > 3
