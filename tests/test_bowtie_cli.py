"""The bowtie front end (mirge_amd/bowtie.py) on the CPU: the nine bowtie command shapes of the reference parse to the
intended policy, anything else is refused, `build` / `inspect` / `install` work without a GPU, and mrg_write_bowtie
formats the model's own alignment arrays byte for byte as tests/bowtie_text_model.py does."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import bowtie_text_model as btm
from tests.conftest import ROOT

# The reference's bowtie calls (runAnnotationPipeline.py:577-599, writeDataToCSV.py:1263/:1488, miRge2.0.py:538/572/586)
# as flag lists -> (mode, mm, (seed_len, max_mm_seed, max_mm_total), trims, strands, stratum_mode, m, sam)
SHAPES = [
    (["--threads", "4", "-n", "0", "-f", "--norc", "-S"], ("n", 0, (28, 0, 2), (0, 0), 1, "best", 0, True)),
    (["--threads", "4", "-n", "1", "-f", "--norc", "-S"], ("n", 1, (28, 1, 2), (0, 0), 1, "best", 0, True)),
    (["--threads", "4", "-v", "1", "-a", "--best", "--strata", "-f", "--norc", "-S"],
     ("v", 1, (1024, 1, 1), (0, 0), 1, "best", 0, True)),
    (["--threads", "4", "-5", "1", "-3", "2", "-v", "2", "--best", "-f", "--norc", "-S"],
     ("v", 2, (1024, 2, 2), (1, 2), 1, "best", 0, True)),
    (["-n", "1", "-f", "-a", "-3", "2", "--threads", "4"], ("n", 1, (28, 1, 2), (0, 2), 2, "all", 0, False)),
    (["-n", "0", "-f", "-a", "-3", "2", "--threads", "4"], ("n", 0, (28, 0, 2), (0, 2), 2, "all", 0, False)),
    (["--threads", "4", "-f", "-n", "0", "-m", "3", "-l", "25", "-S", "-a", "--best"],
     ("n", 0, (25, 0, 2), (0, 0), 2, "all", 3, True)),
    (["--threads", "4", "-f", "-n", "0", "-l", "25", "-a", "--best", "--norc", "-S"],
     ("n", 0, (25, 0, 2), (0, 0), 1, "all", 0, True)),
    (["--threads", "4", "--phred64-quals", "-f", "-n", "1", "-l", "15", "-5", "1", "-3", "3", "-a", "--best", "--strata",
      "--norc", "-S"], ("n", 1, (15, 1, 2), (1, 3), 1, "best", 0, True)),
]


def rnd(rng, n):
    return "".join("ACGT"[c] for c in rng.integers(0, 4, n))


def revcomp(s):
    return s[::-1].translate(str.maketrans("ACGTN", "TGCAN"))


def mutate(rng, s, k):
    s = list(s)
    for i in rng.choice(len(s), size=min(k, len(s)), replace=False):
        s[i] = "ACGTN"[(("ACGTN".index(s[i]) + 1 + int(rng.integers(0, 3))) % 4)]
    return "".join(s)


def random_world(seed, n_parts=2, entries=4, entry_len=(300, 1500), n_reads=300, repeat_copies=12, n_runs=True):
    """(parts, reads FASTA text): entries with N runs, a repeated element (copies on both strands and across parts),
    a palindrome, reads drawn from the entries on either strand with 0-3 substitutions, some with N, some random."""
    rng = np.random.default_rng(seed)
    elem = rnd(rng, 24)
    half = rnd(rng, 11)
    pal = half + revcomp(half)
    parts = []
    for p in range(n_parts):
        names, seqs = [], []
        for e in range(entries):
            s = rnd(rng, int(rng.integers(*entry_len)))
            for _ in range(repeat_copies // (n_parts * entries) + 1):
                at = int(rng.integers(0, len(s) - 30))
                s = s[:at] + (elem if rng.random() < 0.5 else revcomp(elem)) + s[at:]
            at = int(rng.integers(0, len(s) - 30))
            s = s[:at] + pal + s[at:]
            if n_runs and rng.random() < 0.5:
                at = int(rng.integers(0, len(s) - 10))
                s = s[:at] + "N" * int(rng.integers(1, 6)) + s[at + 3:]
            names.append("p%de%d" % (p, e))
            seqs.append(s)
        parts.append((names, seqs))
    allseq = [s for _, ss in parts for s in ss]
    lines = []
    for r in range(n_reads):
        L = int(rng.integers(16, 36))
        kind = rng.random()
        if kind < 0.1:
            q = rnd(rng, L)
        elif kind < 0.2:
            q = elem[:min(L, 24)] + rnd(rng, max(0, L - 24))
        elif kind < 0.25:
            q = pal
        else:
            src = allseq[int(rng.integers(0, len(allseq)))]
            at = int(rng.integers(0, len(src) - L))
            q = src[at:at + L].replace("N", "A")
            q = mutate(rng, q, int(rng.choice([0, 0, 1, 1, 2, 3])))
            if rng.random() < 0.5:
                q = revcomp(q)
        if rng.random() < 0.05:
            i = int(rng.integers(0, len(q)))
            q = q[:i] + "N" + q[i + 1:]
        lines.append(">r%d extra words\n%s\n" % (r, q if rng.random() < 0.9 else q.lower()))
    return parts, "".join(lines)


def shim(*args, timeout=120, env=None):
    return subprocess.run([sys.executable, "-m", "mirge_amd.bowtie"] + list(args), cwd=ROOT, capture_output=True, text=True,
                          timeout=timeout, env=env)


@pytest.mark.parametrize("flags,want", SHAPES)
def test_reference_shapes_parse(flags, want):
    from mirge_amd import bowtie
    o = bowtie.parse_align(flags + ["idx", "reads.fa", "out.sam"])
    assert (o.mode, o.mm, o.seed, o.trims, o.strands, o.stratum_mode, o.m, o.sam) == want
    assert (o.index, o.reads, o.out) == ("idx", "reads.fa", "out.sam")
    assert o.k1 == ("-a" not in flags)
    assert bowtie.parse_align(flags + ["idx", "reads.fa"]).out is None


@pytest.mark.parametrize("bad", [["-x"], ["-p", "4"], ["-q"], ["-k", "2"], ["-n"], ["-n", "one"], ["--sam"], []])
def test_unknown_or_bad_option_exits_1(bad):
    argv = ["-f"] + bad + (["idx", "reads.fa"] if bad else [])
    r = shim("align", *argv, timeout=60)
    assert r.returncode == 1
    assert "usage: bowtie" in r.stderr
    assert r.stdout == ""


def test_unknown_command_exits_1():
    assert shim("frobnicate", timeout=60).returncode == 1


def test_build_then_inspect_round_trip(native_lib, tmp_path):
    parts, _ = random_world(5, n_parts=1)
    names, seqs = parts[0]
    fa = tmp_path / "lib.fa"
    fa.write_text("".join(">%s some description\n%s\n" % (n, s) for n, s in zip(names, seqs)))
    prefix = str(tmp_path / "idx")
    assert shim("build", "-f", str(fa), prefix).returncode == 0
    assert os.path.isfile(prefix + ".mrgfm")
    r = shim("inspect", "-n", prefix)
    assert r.returncode == 0 and r.stdout == "".join(n + "\n" for n in names)
    r = shim("inspect", prefix)
    assert r.returncode == 0 and r.stdout == "".join(">%s\n%s\n" % (n, s) for n, s in zip(names, seqs))


def test_install_writes_three_programs(native_lib, tmp_path):
    d = tmp_path / "bin"
    assert shim("install", str(d)).returncode == 0
    for prog in ("bowtie", "bowtie-build", "bowtie-inspect"):
        p = d / prog
        assert p.is_file() and os.access(p, os.X_OK)
        assert p.read_text().startswith("#!" + sys.executable + "\n")
    fa = tmp_path / "lib.fa"
    fa.write_text(">a\nACGTACGTAC\n>b\nGGGGCCCCAAAATTTT\n")
    env = dict(os.environ, PYTHONPATH="")
    r = subprocess.run([str(d / "bowtie-build"), "-f", str(fa), str(tmp_path / "x")], capture_output=True, text=True,
                       timeout=120, env=env, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(d / "bowtie-inspect"), "-n", str(tmp_path / "x")], capture_output=True, text=True, timeout=120,
                       env=env, cwd=str(tmp_path))
    assert r.returncode == 0 and r.stdout == "a\nb\n"
    r = subprocess.run([str(d / "bowtie"), "-f", "-k", "3", "x", "y"], capture_output=True, text=True, timeout=120, env=env,
                       cwd=str(tmp_path))
    assert r.returncode == 1 and "usage" in r.stderr


@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("shape", range(len(SHAPES)))
def test_writer_matches_model_text(native_lib, oracle_lib, tmp_path, seed, shape):
    from mirge_amd import bowtie
    from mirge_amd.index import FmIndex
    parts, fasta = random_world(100 * seed + shape)
    flags = SHAPES[shape][0]
    if seed == 3 and "-m" not in flags:     # -m suppression on other shapes too
        flags = flags + ["-m", "2"]
    argv = flags + ["idx", "reads.fa"]
    want_out, want_err = btm.run(argv, parts, fasta)
    names, qs, off, entry, offset, strand, mm, supp = btm.arrays(argv, parts, fasta)
    assert len(entry) > 0
    ix = [FmIndex.build(n, s) for n, s in parts]
    o = bowtie.parse_align(argv)
    out = tmp_path / "out.txt"
    s = bowtie.write_bowtie(str(out), o.sam, "bowtie " + " ".join(argv), ix, names, qs, np.array(off), np.array(entry),
                            np.array(offset), np.array(strand), np.array(mm), np.array(supp), o.m)
    assert out.read_text() == want_out
    assert bowtie.summary_text(s, o.m > 0) == want_err


def test_writer_block_threads_give_the_same_bytes(native_lib, oracle_lib, tmp_path):
    """More reads than one formatting block, several workers vs one."""
    from mirge_amd import bowtie
    from mirge_amd.index import FmIndex
    parts, _ = random_world(9, n_reads=1)
    names, seqs = parts[0]
    rng = np.random.default_rng(4)
    n = 70000
    e = rng.integers(0, len(names), n)
    o = np.array([int(rng.integers(0, 200)) for _ in range(n)])
    qs = [seqs[a][b:b + 20] for a, b in zip(e, o)]
    keep = np.array(["N" not in q for q in qs])
    off = np.concatenate([[0], np.cumsum(keep)])
    ix = [FmIndex.build(*parts[0])]
    outs = []
    for th in ("1", "7"):
        os.environ["MIRGE_AMD_TABLE_THREADS"] = th
        try:
            p = tmp_path / ("o%s.sam" % th)
            bowtie.write_bowtie(str(p), True, "x", ix, ["r%d" % i for i in range(n)], qs, off, e[keep], o[keep],
                                np.zeros(int(keep.sum()), np.uint8), np.zeros(int(keep.sum()), np.uint8),
                                np.zeros(n, bool), 0)
            outs.append(p.read_bytes())
        finally:
            del os.environ["MIRGE_AMD_TABLE_THREADS"]
    assert outs[0] == outs[1] and outs[0].count(b"\n") == n + 2 + len(names)


def test_long_read_exits_1_naming_the_limit(native_lib, tmp_path):
    fa = tmp_path / "lib.fa"
    fa.write_text(">a\n" + "ACGT" * 100 + "\n")
    assert shim("build", str(fa), str(tmp_path / "x")).returncode == 0
    reads = tmp_path / "r.fa"
    reads.write_text(">r\n" + "ACGT" * 64 + "\n")
    r = shim("align", "-f", "-n", "0", str(tmp_path / "x"), str(reads))
    assert r.returncode == 1 and "255" in r.stderr
