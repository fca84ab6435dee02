"""The bowtie front end on the GPU (-m gpu): `python -m mirge_amd.bowtie align` run as a fresh process for each of the
reference's nine bowtie shapes prints exactly what tests/bowtie_text_model.py (oracle.model's exhaustive scan, plain
Python text) prints -- on small libraries and on a synthetic genome in three parts with a 10^4-copy element, a 40-copy
element, palindromes and reads with N; `-m` over the parts equals `-m` over the same genome as one library; and
Engine.list_valid agrees with Engine.list_best where both apply."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import bowtie_text_model as btm
from tests.conftest import ROOT
from tests.test_bowtie_cli import SHAPES, random_world, revcomp, rnd, mutate

pytestmark = pytest.mark.gpu

PART_BASES = 1 << 20
BIG_COPIES = 10000


def genome_world(seed, n_reads=500):
    """Three parts of ~1 Mbp (several entries each, N runs); a 25-nt element with 10^4 copies on both strands spread
    over the parts, a 30-nt element with 40 copies, palindromes; reads from all of it."""
    rng = np.random.default_rng(seed)
    big, mid = rnd(rng, 25), rnd(rng, 30)
    pals = [(lambda h: h + revcomp(h))(rnd(rng, 10)) for _ in range(4)]
    parts = []
    for p in range(3):
        names, seqs = [], []
        for e in range(4):
            chunks, n = [], 0
            while n < PART_BASES // 4:
                k = int(rng.integers(20, 200))
                chunks.append(rnd(rng, k))
                n += k
                x = rng.random()
                if x < BIG_COPIES / 3 / 4 / (PART_BASES / 4 / 110):
                    chunks.append(big if rng.random() < 0.5 else revcomp(big))
                elif x < 0.9 and rng.random() < 0.003:
                    chunks.append(mid if rng.random() < 0.5 else revcomp(mid))
                elif rng.random() < 0.001:
                    chunks.append(pals[int(rng.integers(0, 4))])
                elif rng.random() < 0.0005:
                    chunks.append("N" * int(rng.integers(1, 30)))
            names.append("chr%d_%d" % (p, e))
            seqs.append("".join(chunks))
        parts.append((names, seqs))
    allseq = [s for _, ss in parts for s in ss]
    reads = []
    for r in range(n_reads):
        L = int(rng.integers(16, 26))
        x = rng.random()
        if r < 2:
            q = big[:L]
        elif x < 0.05:
            q = mid[:L]
        elif x < 0.1:
            q = pals[int(rng.integers(0, 4))] + rnd(rng, max(0, L - 20))
        elif x < 0.2:
            q = rnd(rng, L)
        else:
            src = allseq[int(rng.integers(0, len(allseq)))]
            at = int(rng.integers(0, len(src) - L))
            q = mutate(rng, src[at:at + L].replace("N", "C"), int(rng.choice([0, 0, 0, 1, 1, 2])))
            if rng.random() < 0.5:
                q = revcomp(q)
        if rng.random() < 0.04:
            i = int(rng.integers(0, L))
            q = q[:i] + "N" + q[i + 1:]
        reads.append(">g%d\n%s\n" % (r, q))
    return parts, "".join(reads)


def write_parts(parts, prefix):
    from mirge_amd.index import FmIndex
    for k, (names, seqs) in enumerate(parts):
        FmIndex.build(names, seqs).save("%s.part%03d.mrgfm" % (prefix, k))


def shim_align(argv, timeout=600):
    r = subprocess.run([sys.executable, "-m", "mirge_amd.bowtie", "align"] + argv, cwd=ROOT, capture_output=True, text=True,
                       timeout=timeout)
    assert r.returncode == 0, r.stderr[-2000:]
    # (the summary is the front end's whole stderr; a line the GPU runtime itself may print at start-up is not)
    err = r.stderr
    at = err.find("# reads processed:")
    assert at >= 0, err[-2000:]
    return r.stdout, err[at:]


@pytest.fixture(scope="module")
def small(tmp_path_factory, native_lib, oracle_lib):
    d = tmp_path_factory.mktemp("small")
    parts, fasta = random_world(2024, n_parts=2, entries=6, n_reads=600)
    write_parts(parts, str(d / "lib"))
    (d / "reads.fa").write_text(fasta)
    return d, parts, fasta


@pytest.fixture(scope="module")
def genome(tmp_path_factory, native_lib, oracle_lib):
    d = tmp_path_factory.mktemp("genome")
    parts, fasta = genome_world(77)
    write_parts(parts, str(d / "g"))
    (d / "reads.fa").write_text(fasta)
    return d, parts, fasta


@pytest.mark.parametrize("shape", range(len(SHAPES)))
def test_shim_equals_model_small_libraries(small, shape):
    d, parts, fasta = small
    argv = SHAPES[shape][0] + [str(d / "lib"), str(d / "reads.fa")]
    out, err = shim_align(argv)
    want_out, want_err = btm.run(argv, parts, fasta)
    assert out == want_out
    assert err == want_err


@pytest.mark.parametrize("shape", range(len(SHAPES)))
def test_shim_equals_model_genome_parts(genome, shape, tmp_path):
    d, parts, fasta = genome
    argv = SHAPES[shape][0] + [str(d / "g"), str(d / "reads.fa"), str(tmp_path / "out.txt")]
    out, err = shim_align(argv)
    assert out == ""
    want_out, want_err = btm.run(argv[:-1], parts, fasta)
    assert (tmp_path / "out.txt").read_text() == want_out.replace(
        'CL:"bowtie %s"' % " ".join(argv[:-1]), 'CL:"bowtie %s"' % " ".join(argv))
    assert err == want_err


def test_m_over_parts_equals_one_library(genome, tmp_path):
    d, parts, fasta = genome
    from mirge_amd.index import FmIndex
    names = [n for ns, _ in parts for n in ns]
    seqs = [s for _, ss in parts for s in ss]
    FmIndex.build(names, seqs).save(str(tmp_path / "whole.mrgfm"))
    flags = SHAPES[6][0]
    a, ea = shim_align(flags + [str(d / "g"), str(d / "reads.fa")])
    b, eb = shim_align(flags + [str(tmp_path / "whole"), str(d / "reads.fa")])
    drop_pg = lambda t: "".join(l for l in t.splitlines(True) if not l.startswith("@PG"))
    assert drop_pg(a) == drop_pg(b) and ea == eb
    assert "suppressed due to -m: 0 " not in ea   # (the 10^4- and 40-copy reads are suppressed)


def test_ten_thousand_copies_are_all_listed(genome, tmp_path):
    d, parts, fasta = genome
    first = fasta.splitlines()[1]
    (tmp_path / "one.fa").write_text(">big\n%s\n" % first)
    argv = ["-n", "1", "-f", "-a", "-3", "2", str(d / "g"), str(tmp_path / "one.fa")]
    out, err = shim_align(argv)
    lines = out.splitlines()
    assert len(lines) >= BIG_COPIES * 0.9
    assert {l.split("\t")[1] for l in lines} == {"+", "-"}
    want_out, want_err = btm.run(argv, parts, (tmp_path / "one.fa").read_text())
    assert out == want_out and err == want_err


def test_list_valid_best_forward_equals_list_best(small):
    d, parts, fasta = small
    from mirge_amd import pack
    from mirge_amd.engine import Engine, ReadSet, STRATUM_BEST
    from mirge_amd.index import FmIndex
    names, seqs = btm.read_fasta(fasta)
    words, lens, nmask = pack.pack_reads(seqs)
    eng = Engine(0)
    try:
        ix = FmIndex.build(*parts[0])
        eng.add_library("lib", ix)
        rs = ReadSet(words, lens, nmask, device=eng.device)
        for seed_len, ms, mt in ((28, 0, 2), (28, 1, 2), (1024, 1, 1), (15, 1, 2)):
            best_mm, off_b, ref_b, pos_b = eng.list_best(rs, "lib", seed_len=seed_len, max_mm_seed=ms, max_mm_total=mt)
            off, entry, offset, strand, mm, supp = eng.list_valid(rs, ["lib"], strands=1, stratum_mode=STRATUM_BEST,
                                                                  seed_len=seed_len, max_mm_seed=ms, max_mm_total=mt)
            assert not supp.any() and not strand.any()
            n_listed = 0
            for r in range(len(seqs)):
                a = set(zip(ref_b[off_b[r]:off_b[r + 1]].tolist(), pos_b[off_b[r]:off_b[r + 1]].tolist()))
                b = set(zip(entry[off[r]:off[r + 1]].tolist(), offset[off[r]:off[r + 1]].tolist()))
                assert a == b, (r, seqs[r])
                if b:
                    assert set(mm[off[r]:off[r + 1]].tolist()) == {int(best_mm[r])}
                n_listed += len(b)
            assert n_listed > 0
    finally:
        eng.close()
