"""`annotate -tcf` on the GPU: Engine.seq_rank (mrg_seq_rank, csrc/collapsed_order.hip) against Python's string order on
hand-made read sets, Engine.collapsed_order (mrg_collapsed_order) against the model of the file's order
(tests/collapsed_order_model.py), the argument checks of both calls, and `annotate -tcf` end to end with and without
--tcf-host.  Everything is compared for equality."""
import ctypes as C
import json
import os
import types

import numpy as np
import pytest

from mirge_amd import pack
from tests import collapsed_order_model as model
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu

BOUNDARY_BASES = (1, 21, 22, 32, 33, 42, 43, 64)             # 1-based: the chunk (21) and packed-word (32) boundaries
EXACT_LENGTHS = (21, 22, 42, 43, 63, 64, 65, 128, 129, 255)
SIZES = (1, 63, 64, 65, 4096, 4097, 65537)                   # across the radix tiles and the scan levels


@pytest.fixture(scope="module")
def engine(native_lib):
    from mirge_amd.engine import Engine
    return Engine(0)


def rand_seq(rng, L, alphabet="ACGT"):
    return "".join(alphabet[i] for i in rng.integers(0, len(alphabet), L))


def differing_at(rng, L, base_1):
    """Five reads of L nt that differ at base base_1 only: A / C / G / N / T there."""
    r = rand_seq(rng, L)
    return [r[:base_1 - 1] + x + r[base_1:] for x in "ACGNT"]


def hand_made_reads():
    rng = np.random.default_rng(2024)
    r16 = rand_seq(rng, 16)
    reads = ["", r16] + [r16 + x for x in "ACGNT"]            # a zero-length read; prefix order and the end code
    for base in BOUNDARY_BASES:
        reads += differing_at(rng, max(base, 16) + int(rng.integers(0, 9)), base)
        reads += differing_at(rng, base, base)               # ... the differing base the last one
    for L in EXACT_LENGTHS:
        r = rand_seq(rng, L, "ACGTN")
        reads += [r, r[:-1], r[:-1] + ("A" if r[-1] != "A" else "T")]
    last = rand_seq(rng, 254)
    reads += [last + "C", last + "G"]                        # 255 nt, the last base alone: every chunk takes part
    for c in range(13):                                      # ... and a pair per chunk
        reads += differing_at(rng, 255, 21 * c + 1 + int(rng.integers(0, 21 if c < 12 else 3)))[:2]
    reads = list(dict.fromkeys(reads))
    return [reads[i] for i in rng.permutation(len(reads))]


HAND_MADE = hand_made_reads()


def with_garbage(rng, words, lens, nmask):
    """The same reads with random bits in the words and the mask at and beyond each length."""
    W, n = words.shape
    nb = np.clip(lens.astype(np.int64)[None, :] - 32 * np.arange(W)[:, None], 0, 32)
    keep = np.where(nb >= 32, np.uint64(2 ** 64 - 1), (np.uint64(1) << (2 * nb).astype(np.uint64)) - np.uint64(1))
    noise = rng.integers(0, 2 ** 64, size=(2, W, n), dtype=np.uint64)
    nm = np.zeros_like(words) if nmask is None else nmask
    return (words & keep) | (noise[0] & ~keep), (nm & keep) | (noise[1] & ~keep)


def ranks_of(engine, words, lens, nmask, max_len=None):
    return engine.seq_rank(words, lens, nmask, max_len).cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("garbage", [False, True])
@pytest.mark.parametrize("W", [1, 2, 4, 8])
def test_seq_rank_on_the_hand_made_reads(engine, W, garbage):
    seqs = [s for s in HAND_MADE if len(s) <= min(255, 32 * W)]
    assert len(seqs) > 40 and "" in seqs and max(map(len, seqs)) == min(255, 32 * W)
    words, lens, nmask = pack.pack_reads(seqs, W)
    assert words.shape[0] == W and nmask is not None
    if garbage:
        clean = words, nmask
        words, nmask = with_garbage(np.random.default_rng(W), words, lens, nmask)
        assert not np.array_equal(words, clean[0]) and not np.array_equal(nmask, clean[1])
    want = model.string_rank(seqs)
    assert np.array_equal(ranks_of(engine, words, lens, nmask), want)
    # a bound above the longest read changes the number of chunks, not the ranks
    assert np.array_equal(ranks_of(engine, words, lens, nmask, min(255, 32 * W)), want)


def test_seq_rank_without_a_mask_and_with_garbage_in_the_words(engine):
    rng = np.random.default_rng(5)
    seqs = [s for s in HAND_MADE if "N" not in s]
    words, lens, nmask = pack.pack_reads(seqs, 8)
    assert nmask is None
    want = model.string_rank(seqs)
    assert np.array_equal(ranks_of(engine, words, lens, None), want)
    assert np.array_equal(ranks_of(engine, with_garbage(rng, words, lens, None)[0], lens, None), want)


def test_seq_rank_every_chunk_takes_part(engine):
    """Two 255-nt reads that differ only in the last base, in both array orders."""
    r = rand_seq(np.random.default_rng(9), 254)
    for seqs in ([r + "A", r + "T"], [r + "T", r + "A"], [r + "N", r + "G"], [r, r + "A"]):
        words, lens, nmask = pack.pack_reads(seqs, 8)
        assert np.array_equal(ranks_of(engine, words, lens, nmask), model.string_rank(seqs)), seqs


@pytest.fixture(scope="module")
def world():
    """65 537 distinct reads of 16-40 nt, some with N, and zipf counts over two samples (made once, left unchanged)."""
    rng = np.random.default_rng(65537)
    seqs = model.random_reads(rng, SIZES[-1])
    quant = np.minimum(rng.zipf(1.5, size=(len(seqs), 2)), 2 ** 32 - 1).astype(np.uint32)
    quant[rng.random(quant.shape) < 0.35] = 0
    words, lens, nmask = pack.pack_reads(seqs, 2)
    return types.SimpleNamespace(seqs=seqs, quant=quant, words=words, lens=lens, nmask=nmask)


@pytest.mark.parametrize("n", SIZES)
def test_seq_rank_random_reads(engine, world, n):
    seqs = world.seqs[:n]
    got = ranks_of(engine, np.ascontiguousarray(world.words[:, :n]), world.lens[:n], np.ascontiguousarray(world.nmask[:, :n]))
    assert np.array_equal(got, model.string_rank(seqs))


def test_seq_rank_equal_reads_still_give_a_permutation(engine):
    rng = np.random.default_rng(3)
    seqs = model.random_reads(rng, 300) * 3 + [""] * 4
    words, lens, nmask = pack.pack_reads(seqs, 2)
    got = ranks_of(engine, words, lens, nmask)
    assert np.array_equal(np.sort(got), np.arange(len(seqs)))
    assert [seqs[u] for u in np.argsort(got)] == sorted(seqs)


def orders_equal_model(engine, seqs, quant, W=None, on_device=False):
    words, lens, nmask = pack.pack_reads(seqs, W)
    quant = np.ascontiguousarray(quant, dtype=np.uint32)
    if on_device:
        from mirge_amd.engine import ReadSet
        rs = ReadSet(words, lens, nmask, quant, device=engine.device)
        got = engine.collapsed_order(rs.words, rs.lens, rs.nmask, rs.quant)
    else:
        got = engine.collapsed_order(words, lens, nmask, quant)
    assert len(got) == quant.shape[1]
    for s, order in enumerate(got):
        assert order.dtype == np.uint32 and order.shape == (int(np.count_nonzero(quant[:, s])),), s
        assert np.array_equal(order, model.order(seqs, quant[:, s])), s
    return got


def test_order_all_counts_one(engine):
    seqs = HAND_MADE
    orders_equal_model(engine, seqs, np.ones((len(seqs), 1), np.uint32))
    orders_equal_model(engine, seqs, np.ones((len(seqs), 1), np.uint32), on_device=True)


def test_order_counts_over_the_whole_uint32_range(engine):
    rng = np.random.default_rng(11)
    counts = [1, 255, 256, 65535, 65536, 2 ** 31, 2 ** 32 - 1]
    seqs = model.random_reads(rng, 5 * len(counts))          # five reads tie on every count: the string decides
    quant = np.array([counts[i % len(counts)] for i in range(len(seqs))], dtype=np.uint32)[:, None]
    got = orders_equal_model(engine, seqs, quant)
    assert quant[got[0][0], 0] == 2 ** 32 - 1 and quant[got[0][-1], 0] == 1
    assert quant[got[0][5], 0] == 2 ** 31


def test_order_leaves_out_the_reads_without_a_count(engine):
    rng = np.random.default_rng(12)
    seqs = model.random_reads(rng, 700)
    quant = rng.integers(0, 4, (len(seqs), 1)).astype(np.uint32)
    got = orders_equal_model(engine, seqs, quant)
    assert 0 < got[0].shape[0] < len(seqs) and not np.any(quant[got[0], 0] == 0)


def test_order_of_a_column_that_is_all_zero(engine):
    rng = np.random.default_rng(13)
    seqs = model.random_reads(rng, 130)
    quant = np.zeros((len(seqs), 2), np.uint32)
    quant[:, 1] = rng.integers(1, 9, len(seqs))
    got = orders_equal_model(engine, seqs, quant)
    assert got[0].shape == (0,) and got[1].shape == (len(seqs),)


def test_order_three_samples_with_different_supports(engine):
    rng = np.random.default_rng(14)
    seqs = model.random_reads(rng, 1000, lo=1, hi=90)
    quant = rng.integers(1, 6, (len(seqs), 3)).astype(np.uint32)
    quant[: 400, 0] = 0
    quant[300: 900, 1] = 0
    quant[::3, 2] = 0
    orders_equal_model(engine, seqs, quant)
    orders_equal_model(engine, seqs, quant, on_device=True)


def test_order_of_the_zipf_world_and_its_files(engine, world, tmp_path):
    from mirge_amd import columnar
    timings = {}
    got = engine.collapsed_order(world.words, world.lens, world.nmask, world.quant, timings=timings)
    for s in range(2):
        assert np.array_equal(got[s], model.order(world.seqs, world.quant[:, s])), s
    assert timings["rank_ms"] > 0 and timings["order_ms"] > 0
    samples = ["a.fastq", "b.fastq"]
    columnar.write_collapsed_fa(str(tmp_path), samples, world.words, world.lens, world.nmask, world.quant, got, {})
    for s, fn in enumerate(("a.trim.collapse.fa", "b.trim.collapse.fa")):
        assert (tmp_path / fn).read_bytes() == model.text(world.seqs, world.quant[:, s]), fn


def test_no_reads_give_empty_orders(engine):
    got = engine.collapsed_order(np.zeros((1, 0), np.uint64), np.zeros(0, np.uint8), None, np.zeros((0, 2), np.uint32))
    assert [o.shape for o in got] == [(0,), (0,)]


def test_argument_checks(engine):
    import torch
    from mirge_amd._native import MRG_ERR_ARG
    L, h, st = engine._lib, engine._h, engine._stream_ptr()
    seqs = ["ACGTACGTACGTACGTACGTAC", "ACGTACGTACGTACGTA", "TTTTACGTACGTACGTAC"]
    words, lens, nmask = pack.pack_reads(seqs, 1)
    d_words = torch.from_numpy(words.view(np.int64)).to(engine.device)
    d_lens = torch.from_numpy(lens).to(engine.device)
    d_quant = torch.tensor([[3, 0], [3, 1], [0, 2]], dtype=torch.int32, device=engine.device)
    need_r, need_o = C.c_uint64(), C.c_uint64()
    assert L.mrg_collapsed_order_temp_bytes(3, C.byref(need_r), C.byref(need_o)) == 0
    tmp = torch.empty(int(max(need_r.value, need_o.value)), dtype=torch.uint8, device=engine.device)
    d_rank = torch.empty(3, dtype=torch.int32, device=engine.device)
    d_order = torch.full((3,), -1, dtype=torch.int32, device=engine.device)
    w, l, q, r, o, t = (x.data_ptr() for x in (d_words, d_lens, d_quant, d_rank, d_order, tmp))

    def refused(rc, word):
        assert rc == MRG_ERR_ARG and word in L.mrg_last_error(), (rc, L.mrg_last_error())
    refused(L.mrg_seq_rank(h, w, 1, 3, l, None, 0, 22, r, t, tmp.numel(), st), b"no reads")
    refused(L.mrg_seq_rank(h, w, 3, 3, l, None, 3, 22, r, t, tmp.numel(), st), b"words_per_read")
    refused(L.mrg_seq_rank(h, w, 1, 2, l, None, 3, 22, r, t, tmp.numel(), st), b"stride")
    refused(L.mrg_seq_rank(h, w, 1, 3, l, None, 3, 33, r, t, tmp.numel(), st), b"max_len")
    refused(L.mrg_seq_rank(h, w, 1, 3, l, None, 3, 22, r, t, need_r.value - 1, st), b"scratch")
    refused(L.mrg_seq_rank(h, w, 1, 3, l, None, 3, 21, r, t, tmp.numel(), st), b"longer than max_len")   # (found on the device)
    for hole in range(4):
        a = [w, l, r, t]
        a[hole] = None
        refused(L.mrg_seq_rank(h, a[0], 1, 3, a[1], None, 3, 22, a[2], a[3], tmp.numel(), st), b"null")
    assert L.mrg_seq_rank(h, w, 1, 3, l, None, 3, 22, r, t, tmp.numel(), st) == 0
    assert d_rank.cpu().tolist() == [1, 0, 2]
    rows = C.c_uint64(99)
    refused(L.mrg_collapsed_order(h, q, 0, 2, 0, r, o, 3, C.byref(rows), t, tmp.numel(), st), b"reads")
    refused(L.mrg_collapsed_order(h, q, 3, 0, 0, r, o, 3, C.byref(rows), t, tmp.numel(), st), b"sample 0 of 0")
    refused(L.mrg_collapsed_order(h, q, 3, 2, 2, r, o, 3, C.byref(rows), t, tmp.numel(), st), b"sample 2 of 2")
    refused(L.mrg_collapsed_order(h, q, 3, 2, 0, r, o, 3, C.byref(rows), t, need_o.value - 1, st), b"scratch")
    refused(L.mrg_collapsed_order(h, q, 3, 2, 0, r, o, 3, None, t, tmp.numel(), st), b"null")
    refused(L.mrg_collapsed_order(h, None, 3, 2, 0, r, o, 3, C.byref(rows), t, tmp.numel(), st), b"null")
    refused(L.mrg_collapsed_order(h, q, 3, 2, 0, None, o, 3, C.byref(rows), t, tmp.numel(), st), b"null")
    refused(L.mrg_collapsed_order(h, q, 3, 2, 0, r, None, 3, C.byref(rows), t, tmp.numel(), st), b"null")
    refused(L.mrg_collapsed_order(h, q, 3, 2, 0, r, o, 3, C.byref(rows), None, tmp.numel(), st), b"null")
    # a buffer smaller than the rows: the count comes back, no row is written
    refused(L.mrg_collapsed_order(h, q, 3, 2, 0, r, o, 1, C.byref(rows), t, tmp.numel(), st), b"do not fit")
    assert rows.value == 2 and d_order.cpu().tolist() == [-1, -1, -1]
    assert L.mrg_collapsed_order(h, q, 3, 2, 0, r, o, 2, C.byref(rows), t, tmp.numel(), st) == 0
    assert rows.value == 2 and d_order.cpu().tolist() == [0, 1, -1]       # count 3 twice: the longer read first
    assert L.mrg_collapsed_order(h, q, 3, 2, 1, r, o, 3, C.byref(rows), t, tmp.numel(), st) == 0
    assert rows.value == 2 and d_order.cpu().tolist()[:2] == [2, 1]


def test_cli_tcf_with_and_without_tcf_host(native_lib, tmp_path, monkeypatch):
    """Two samples, reads with N, one read beyond 255 nt in both samples: the files of the array route, of --tcf-host and
    of the model are the same bytes, and the array route builds no Python object per read."""
    from mirge_amd import cli, report, synth
    with open(os.path.join(ROOT, "tests", "golden", "flags.json")) as fh:
        golden = json.load(fh)
    ns = types.SimpleNamespace(libs={k: tuple(v) for k, v in golden["libraries"].items()}, merges=golden["merges"])
    root = str(tmp_path / "libs")
    synth.SynthLibraries.write_layout(ns, root, species="syn", db="miRBase")
    rng = np.random.default_rng(21)
    long_read = rand_seq(rng, 300)
    with_n = [s[:5] + "N" + s[6:] for s in model.random_reads(rng, 30, lo=18, hi=60, p_n=0.0)]
    samples, fastqs = [], []
    for i, (name, reads) in enumerate(zip(golden["sample_list"], golden["samples"])):
        reads = list(reads) + [long_read] * (2 + i) + [r for k, r in enumerate(with_n) for _ in range(1 + (k + i) % 3)]
        reads += [long_read[:254]] * (2 + i)                  # (a packed read that ties with the long one on the count)
        samples.append(reads)
        fastqs.append(str(tmp_path / name))
        with open(fastqs[-1], "w") as fh:
            fh.write("".join("@r%d\n%s\n+\n%s\n" % (k, r, "I" * len(r)) for k, r in enumerate(reads)))

    def run(out, *extra):
        res = cli.annotate_main(cli.build_parser().parse_args(
            ["annotate", "-s"] + fastqs + ["-lib", root, "-sp", "syn", "-o", str(tmp_path / out), "-tcf"] + list(extra)))
        return res["outdir"]
    host = run("host", "--tcf-host")

    def refuse(*a, **k):
        raise AssertionError("the array route took the per-read Python route")
    monkeypatch.setattr(report, "write_collapsed_fa_host", refuse)
    arrays = run("arrays")
    for name, reads in zip(golden["sample_list"], samples):
        fn = os.path.splitext(name)[0] + ".trim.collapse.fa"
        uniq = {}
        for r in reads:
            if len(r) >= 16:
                uniq[r] = uniq.get(r, 0) + 1
        want = model.text(list(uniq), list(uniq.values()))
        with open(os.path.join(host, fn), "rb") as f1, open(os.path.join(arrays, fn), "rb") as f2:
            got = f2.read()
            assert f1.read() == got == want, fn
        assert long_read.encode() in got and b"N" in got
