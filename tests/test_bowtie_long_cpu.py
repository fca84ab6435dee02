"""The bowtie front end's long-read path on the CPU: bowtie.merge_listings puts the packed listing (reads of at most
255 nt) and the ragged one (the others) back into file order; the two C-ABI entry points exist and refuse a null
context by name; mrg_write_bowtie formats 600-nt rows as tests/bowtie_text_model.py does (it holds no length bound);
and `align` admits a read beyond 255 nt only with MIRGE_AMD_LONG_READS=1."""
import numpy as np
import pytest

from tests import bowtie_text_model as btm
from tests.test_bowtie_cli import random_world, revcomp

EMPTY = (np.zeros(1, np.int64), np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.uint8), np.zeros(0, np.uint8),
         np.zeros(0, bool))


def listing(rows_per_read, suppressed, tag):
    """A hand-made listing: read i has rows_per_read[i] rows whose four fields name (tag, i, row) so that each can be
    found again."""
    off = np.zeros(len(rows_per_read) + 1, np.int64)
    np.cumsum(rows_per_read, out=off[1:])
    entry = np.array([tag * 1000 + i for i, k in enumerate(rows_per_read) for _ in range(k)], np.int32)
    offset = np.array([j for k in rows_per_read for j in range(k)], np.int32)
    strand = (offset % 2).astype(np.uint8)
    mm = (offset % 3).astype(np.uint8)
    return off, entry, offset, strand, mm, np.array(suppressed, bool)


def rows_of(lst, i):
    a, b = int(lst[0][i]), int(lst[0][i + 1])
    return [tuple(int(x[t]) for x in lst[1:5]) for t in range(a, b)]


def check_merge(n, idx_a, a, idx_b, b):
    from mirge_amd import bowtie
    got = bowtie.merge_listings(n, np.array(idx_a, np.int64), a, np.array(idx_b, np.int64), b)
    off, entry, offset, strand, mm, supp = got
    assert len(off) == n + 1 and off[0] == 0 and (np.diff(off) >= 0).all()
    assert len(entry) == len(offset) == len(strand) == len(mm) == off[-1]
    assert (entry.dtype, offset.dtype, strand.dtype, mm.dtype, supp.dtype) == (np.int32, np.int32, np.uint8, np.uint8, bool)
    assert len(supp) == n
    seen = set()
    for idx, lst in ((idx_a, a), (idx_b, b)):
        for i, r in enumerate(idx):
            assert rows_of(got, r) == rows_of(lst, i), (r, i)
            assert bool(supp[r]) == bool(lst[5][i])
            seen.add(r)
    for r in set(range(n)) - seen:
        assert off[r + 1] == off[r] and not supp[r]
    return got


@pytest.mark.parametrize("name,n,idx_short,k_short,idx_long,k_long", [
    ("long first", 5, [1, 2, 3, 4], [2, 0, 1, 3], [0], [4]),
    ("long last", 5, [0, 1, 2, 3], [2, 0, 1, 3], [4], [70]),
    ("long adjacent", 7, [0, 1, 5, 6], [1, 1, 0, 2], [2, 3, 4], [3, 0, 5]),
    ("long interleaved", 7, [0, 2, 4, 6], [1, 2, 3, 4], [1, 3, 5], [5, 6, 7]),
    ("no long read", 4, [0, 1, 2, 3], [1, 0, 2, 1], [], []),
    ("all long", 3, [], [], [0, 1, 2], [2, 0, 65]),
    ("no rows at all", 4, [0, 3], [0, 0], [1, 2], [0, 0]),
])
def test_merge_listings_puts_reads_back_in_file_order(name, n, idx_short, k_short, idx_long, k_long):
    a = listing(k_short, [False] * len(k_short), 1) if idx_short else EMPTY
    b = listing(k_long, [False] * len(k_long), 2) if idx_long else EMPTY
    got = check_merge(n, idx_short, a, idx_long, b)
    assert got[0][-1] == sum(k_short) + sum(k_long)


def test_merge_listings_keeps_suppressed_per_read():
    """A suppressed long read (no rows) between aligned short ones, and a suppressed short read next to an aligned
    long one."""
    a = listing([2, 1, 0, 3], [False, False, True, False], 1)
    b = listing([0, 4], [True, False], 2)
    got = check_merge(6, [0, 2, 3, 5], a, [1, 4], b)
    assert got[5].tolist() == [False, True, False, True, False, False]
    assert np.diff(got[0]).tolist() == [2, 0, 1, 0, 4, 3]


def test_merge_listings_of_nothing():
    from mirge_amd import bowtie
    got = bowtie.merge_listings(0, np.zeros(0, np.int64), EMPTY, np.zeros(0, np.int64), EMPTY)
    assert got[0].tolist() == [0] and all(len(x) == 0 for x in got[1:])
    got = check_merge(3, [], EMPTY, [], EMPTY)
    assert got[0].tolist() == [0, 0, 0, 0]


@pytest.mark.parametrize("fn,n_args", [("mrg_list_valid_long_count", 13), ("mrg_list_valid_long_fill", 20)])
def test_symbols_exist_and_refuse_a_null_context(native_lib, fn, n_args):
    from mirge_amd import _native
    assert fn in _native.SIGNATURES and len(_native.SIGNATURES[fn][1]) == n_args
    f = getattr(native_lib, fn)
    args = [None, None, None, None, None, 1, 0, 2, 28, 0, 2]
    args += [None, None] if n_args == 13 else [1, None, None, 0, None, None, None, None, None]
    assert f(*args) != 0
    assert fn in native_lib.mrg_last_error().decode()


def test_writer_formats_600_nt_rows_as_the_model_does(native_lib, oracle_lib, tmp_path):
    """mrg_write_bowtie takes the sequences as a blob with offsets: MD:Z, the mismatch descriptors and the reverse
    complement of 256..600-nt reads, in both formats."""
    from mirge_amd import bowtie
    from mirge_amd.index import FmIndex
    parts, _ = random_world(31, n_parts=2, entries=3, entry_len=(700, 1200), n_reads=1, n_runs=False)
    allseq = [s for _, ss in parts for s in ss]
    lines = []
    for r, L in enumerate((256, 300, 600, 20, 599)):
        src = allseq[r % len(allseq)]
        q = list(src[10:10 + L])
        if L > 30:
            q[L - 7] = "ACGT"[("ACGT".index(q[L - 7]) + 1) % 4]
            q[L // 2] = "N"
        q = "".join(q)
        lines.append(">long%d\n%s\n" % (r, revcomp(q) if r % 2 else q))
    fasta = "".join(lines)
    ix = [FmIndex.build(n, s) for n, s in parts]
    for flags in (["-f", "-v", "2", "-a", "-S"], ["-f", "-v", "2", "-a"]):
        argv = flags + ["idx", "reads.fa"]
        want_out, want_err = btm.run(argv, parts, fasta)
        names, qs, off, entry, offset, strand, mm, supp = btm.arrays(argv, parts, fasta)
        assert len(entry) >= 5 and max(len(q) for q in qs) == 600 and 1 in strand
        o = bowtie.parse_align(argv)
        out = tmp_path / "out.txt"
        s = bowtie.write_bowtie(str(out), o.sam, "bowtie " + " ".join(argv), ix, names, qs, np.array(off), np.array(entry),
                                np.array(offset), np.array(strand), np.array(mm), np.array(supp), o.m)
        assert out.read_text() == want_out
        assert bowtie.summary_text(s, o.m > 0) == want_err


def test_long_reads_are_admitted_only_by_the_environment(native_lib, tmp_path):
    """Without MIRGE_AMD_LONG_READS=1 `align` still exits 1 on a read beyond 255 nt, naming the limit and the variable,
    before it opens the index or the GPU; a batch of short reads is not asked."""
    import os
    from tests.test_bowtie_cli import shim
    reads = tmp_path / "r.fa"
    reads.write_text(">s\nACGTACGTACGTACGTAC\n>r\n" + "ACGT" * 64 + "\n")
    for value in (None, "0", "yes"):
        env = {k: v for k, v in os.environ.items() if k != "MIRGE_AMD_LONG_READS"}
        if value is not None:
            env["MIRGE_AMD_LONG_READS"] = value
        r = shim("align", "-f", "-n", "0", str(tmp_path / "no_such_index"), str(reads), env=env)
        assert r.returncode == 1 and r.stdout == ""
        assert "255" in r.stderr and "MIRGE_AMD_LONG_READS=1" in r.stderr and "256" in r.stderr
    r = shim("align", "-f", "-n", "0", "-3", "1", str(tmp_path / "no_such_index"), str(reads),
             env=dict(os.environ, MIRGE_AMD_LONG_READS="0"))
    assert r.returncode == 1 and "MIRGE_AMD_LONG_READS" not in r.stderr      # (255 nt after -3 1: the index is what is missing)
