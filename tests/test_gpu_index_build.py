"""The device route of the index builder (csrc/sa_build.hip) against the host builder, which is the yardstick: every
array of the index identical, on texts chosen for the places where prefix doubling can go wrong -- suffixes shorter
than the first-round key, suffixes that are prefixes of others, long repeats (many rounds), row counts at the block and
superblock edges, N runs and segment ids.  oracle/index_check.c checks the device-built arrays by definition as well."""
import math
import os

import numpy as np
import pytest

from oracle import model

pytestmark = pytest.mark.gpu

ARRAYS = ("blocks", "super", "text", "sa", "ftab", "seg_start", "seg_ref", "seg_off", "chunk_seg")


def rand_seq(rng, n):
    return "".join("ACGT"[c] for c in rng.integers(0, 4, int(n)))


def round_bound(n):
    """ceil(log2((n + 1) / 30)) + 1; the first-round sort always runs, so never below one."""
    return max(1, math.ceil(math.log2((n + 1) / 30.0)) + 1)


def build_both(names, seqs):
    from mirge_amd.index import FmIndex
    host = FmIndex.build(names, seqs)
    dev = FmIndex.build(names, seqs, device=0)
    rounds = FmIndex.last_device_rounds()
    return host, dev, rounds


def assert_same_index(names, seqs, check=True):
    host, dev, rounds = build_both(names, seqs)
    a, b = host.view(), dev.view()
    for k in ARRAYS:
        assert a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), k
    assert a["ftab_ks"] == b["ftab_ks"]
    for f, _ in host.info._fields_:
        x, y = getattr(host.info, f), getattr(dev.info, f)
        assert (list(x) == list(y)) if hasattr(x, "__len__") else (x == y), f
    for k in ("ctx", "kbits"):
        assert (a[k] is None) == (b[k] is None) and (a[k] is None or np.array_equal(a[k], b[k])), k
    assert dev.names == list(names)
    n = int(dev.info.n_bases)
    assert (1 if n else 0) <= rounds <= round_bound(n), (rounds, n)
    if check:
        model.check_index(b, seqs)
    return host, dev, rounds


def test_entries_shorter_than_the_first_round_key(native_lib, oracle_lib):
    rng = np.random.default_rng(1)
    for L in (1, 5, 29, 30, 31):
        assert_same_index(["e"], [rand_seq(rng, L)])
    assert_same_index(["a", "b", "c", "d", "e"], [rand_seq(rng, L) for L in (1, 5, 29, 30, 31)])
    for s in ("A", "T", "AAAAA", "A" * 29, "A" * 30, "A" * 31, "CAAAA", "ACACACACA"):
        assert_same_index(["e"], [s])


@pytest.mark.parametrize("n", [30, 31, 32, 63, 65534, 65535, 65536, 65537, 131071])
def test_row_count_at_block_and_superblock_edges(native_lib, oracle_lib, n):
    rng = np.random.default_rng(n)
    cut = sorted(rng.integers(0, n + 1, 3).tolist())
    s = rand_seq(rng, n)
    assert_same_index(["a", "b", "c", "d"], [s[:cut[0]], s[cut[0]:cut[1]], s[cut[1]:cut[2]], s[cut[2]:]])


def test_poly_a_needs_every_round(native_lib, oracle_lib):
    n = 70000
    _, _, rounds = assert_same_index(["polyA"], ["A" * n])
    assert rounds == round_bound(n)  # unique only once the width reaches the text's length


def test_short_period_repeat(native_lib, oracle_lib):
    assert_same_index(["acg"], ["ACG" * 20000])


def test_identical_entries_repeat_across_entry_boundaries(native_lib, oracle_lib):
    rng = np.random.default_rng(7)
    e = rand_seq(rng, 3000)
    _, _, rounds = assert_same_index(["x", "y", "gap", "z"], [e, e, rand_seq(rng, 777), e])
    assert rounds >= 8  # a 3000-base repeat cannot be told apart in fewer doublings of 30


def test_suffix_that_is_a_prefix_of_another(native_lib, oracle_lib):
    rng = np.random.default_rng(11)
    for L in (40, 10, 3):  # longer than the first-round key, and inside it
        tail = rand_seq(rng, L - 1) + "G"
        text = rand_seq(rng, 300) + tail + "C" + rand_seq(rng, 200) + tail + "A" * 45 + rand_seq(rng, 150) + tail + "T" + rand_seq(rng, 90) + tail
        assert_same_index(["t"], [text])
        assert_same_index(["t", "u"], [text[:400], text[400:]])
    # the text ends in A's: the last suffixes pad to the same key as each other and as longer runs of A
    text = rand_seq(rng, 500) + "A" * 60 + rand_seq(rng, 500) + "C" + "A" * 35
    assert_same_index(["t"], [text])
    assert_same_index(["t"], [text[:-20]])


def test_n_runs_and_case(native_lib, oracle_lib):
    rng = np.random.default_rng(13)
    names = ["lead", "trail", "only_n", "single", "lower", "empty", "plain"]
    seqs = ["NNN" + rand_seq(rng, 50), rand_seq(rng, 41) + "NN", "NNNNN", "NANCNNGNTN" * 7,
            rand_seq(rng, 80).lower() + "n" + rand_seq(rng, 33), "", rand_seq(rng, 500)]
    host, dev, _ = assert_same_index(names, seqs)
    assert [dev.sequence(i) for i in range(len(seqs))] == [s.upper() for s in seqs]


def test_more_segments_than_a_segment_id_holds(native_lib, oracle_lib):
    rng = np.random.default_rng(17)
    s = np.array(list(rand_seq(rng, 200000)))
    s[2::3] = "N"
    host, dev, _ = assert_same_index(["front", "holes"], [rand_seq(rng, 300), "".join(s)])
    assert dev.info.n_seg > 65535
    assert int(dev.view()["sa"][5]) >> 48 == 0xFFFF


@pytest.mark.parametrize("n", [(1 << 20) - 1, (1 << 20) + 3])
def test_around_the_lazy_derive_threshold(native_lib, oracle_lib, n, monkeypatch, capfd):
    """Below kLazyDeriveBases the host derives ftab / ctx from the device-built rows at once (derived == true); from it
    on both builders leave them planned (derived == false) and the first view derives them, from the same rows.  An
    index says which it is through the stage laps: `derive_tables (host)` runs, and reports, only when derived is
    false."""
    from mirge_amd.index import FmIndex
    monkeypatch.setenv("MIRGE_AMD_TIMING", "1")
    rng = np.random.default_rng(n)
    codes = rng.integers(0, 4, n).astype(np.uint8)
    text = np.frombuffer(b"ACGT", dtype=np.uint8)[codes].tobytes().decode("ascii")
    cuts = [0] + sorted(rng.integers(0, n, 49).tolist()) + [n]
    seqs = [text[cuts[i]:cuts[i + 1]] for i in range(50)]
    names = ["e%d" % i for i in range(50)]
    lazy = n >= (1 << 20)
    for device in (None, 0):
        ix = FmIndex.build(names, seqs, device=device)
        capfd.readouterr()
        ix.view()
        derived_now = "derive_tables (host)" in capfd.readouterr().err
        assert derived_now == lazy, (device, "derived was %s after the build" % (not derived_now))
        ix.view()
        assert "derive_tables (host)" not in capfd.readouterr().err
    assert_same_index(names, seqs)


def test_saved_device_index_serves_count_best_like_the_host_one(native_lib, oracle_lib, tmp_path):
    from mirge_amd import pack
    from mirge_amd.engine import Engine, ReadSet
    from mirge_amd.index import FmIndex
    rng = np.random.default_rng(23)
    seqs = [rand_seq(rng, L) for L in rng.integers(500, 6000, 20)]
    seqs[7] = seqs[3][100:2100] + seqs[7]  # a repeat, so that some reads have several best hits
    names = ["g%d" % i for i in range(20)]
    host, dev, rounds = build_both(names, seqs)
    assert 1 <= rounds <= round_bound(int(dev.info.n_bases))
    host.save(str(tmp_path / "host.mrgfm"))
    dev.save(str(tmp_path / "dev.mrgfm"))
    assert (tmp_path / "host.mrgfm").read_bytes() == (tmp_path / "dev.mrgfm").read_bytes()
    reads = []
    for k in range(2000):
        s = seqs[int(rng.integers(0, 20))]
        o = int(rng.integers(0, len(s) - 24))
        r = list(s[o:o + 22])
        if k & 1:
            j = int(rng.integers(0, 22))
            r[j] = "ACGT"[("ACGT".index(r[j]) + 1 + int(rng.integers(0, 3))) & 3]
        reads.append("".join(r))
    eng = Engine(0)
    eng.add_library("host", FmIndex.load(str(tmp_path / "host.mrgfm")))
    eng.add_library("dev", FmIndex.load(str(tmp_path / "dev.mrgfm")))
    w, l, nm = pack.pack_reads(reads)
    rs = ReadSet(w, l, nm, None, device=eng.device)
    for n_seed in (0, 1):
        mm_h, cnt_h = eng.count_best(rs, "host", seed_len=28, max_mm_seed=n_seed, max_mm_total=1)
        mm_d, cnt_d = eng.count_best(rs, "dev", seed_len=28, max_mm_seed=n_seed, max_mm_total=1)
        assert np.array_equal(np.asarray(mm_h), np.asarray(mm_d)) and np.array_equal(np.asarray(cnt_h), np.asarray(cnt_d))
        assert int((np.asarray(mm_d)[::2] == 0).sum()) == 1000  # the exact reads were found
        assert int((np.asarray(cnt_d) > 1).sum()) > 0


def test_build_index_cli_writes_the_same_part_files(native_lib, tmp_path):
    from mirge_amd import build_index
    rng = np.random.default_rng(29)
    fa = tmp_path / "genome.fa"
    with open(fa, "w") as fh:
        for i in range(7):
            s = rand_seq(rng, 3000 + 500 * i)
            s = s[:1000] + "N" * 20 + s[1020:]
            fh.write(">chr%d\n" % i)
            for o in range(0, len(s), 70):
                fh.write(s[o:o + 70] + "\n")
    assert build_index.main([str(fa), "-o", str(tmp_path / "host"), "--max-bases", "12000"]) == 0
    assert build_index.main([str(fa), "-o", str(tmp_path / "dev"), "--max-bases", "12000", "--device", "0"]) == 0
    from mirge_amd.index import FmIndex
    parts = sorted(p for p in os.listdir(tmp_path) if p.startswith("host.part"))
    assert len(parts) >= 3
    # the counter is the last device build's: the last part's
    assert 1 <= FmIndex.last_device_rounds() <= round_bound(int(FmIndex.load(str(tmp_path / parts[-1])).info.n_bases))
    for p in parts:
        assert (tmp_path / p).read_bytes() == (tmp_path / p.replace("host", "dev", 1)).read_bytes(), p
    assert build_index.main([str(fa), "-o", str(tmp_path / "whole_host")]) == 0
    assert build_index.main([str(fa), "-o", str(tmp_path / "whole_dev"), "--device", "0"]) == 0
    assert 1 <= FmIndex.last_device_rounds() <= round_bound(int(FmIndex.load(str(tmp_path / "whole_dev.mrgfm")).info.n_bases))
    assert (tmp_path / "whole_host.mrgfm").read_bytes() == (tmp_path / "whole_dev.mrgfm").read_bytes()
