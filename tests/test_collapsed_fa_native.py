"""The native writer of <sample>.trim.collapse.fa (mrg_write_collapsed_fasta, columnar.write_collapsed_fa) on the host,
with the order taken from the model (tests/collapsed_order_model.py): byte-equal to the per-read Python route
(report.write_collapsed_fa_host) and to the model's text, the merge of the reads beyond 255 nt, the error paths."""
import ctypes as C
import os

import numpy as np
import pytest

from mirge_amd import columnar, pack, report
from tests import collapsed_order_model as model


def zipf_quant(rng, n, S, p_zero=0.3):
    q = np.minimum(rng.zipf(1.6, size=(n, S)), 2 ** 32 - 1).astype(np.uint32)
    q[rng.random((n, S)) < p_zero] = 0
    return q


def native_write(lib, path, words, lens, nmask, quant, s, order, extra=()):
    """mrg_write_collapsed_fasta on one sample column; extra: (sequence, count) pairs in file order."""
    words = np.ascontiguousarray(words, dtype=np.uint64)
    W, n = words.shape
    lens = np.ascontiguousarray(lens, dtype=np.uint8)
    nm = None if nmask is None else np.ascontiguousarray(nmask, dtype=np.uint64)
    quant = np.ascontiguousarray(quant, dtype=np.uint32)
    order = np.ascontiguousarray(order, dtype=np.uint32)
    seqs = (C.c_char_p * max(len(extra), 1))(*[s_.encode() for s_, _ in extra])
    counts = np.array([c for _, c in extra], dtype=np.uint64)
    return lib.mrg_write_collapsed_fasta(os.fsencode(path), words.ctypes.data, W, n, lens.ctypes.data,
                                         None if nm is None else nm.ctypes.data, n, quant.ctypes.data, quant.shape[1], s,
                                         order.ctypes.data, order.shape[0], seqs, counts.ctypes.data, len(extra))


@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("with_n", [False, True])
@pytest.mark.parametrize("W", [1, 2, 8])
def test_writer_equals_the_host_route(native_lib, tmp_path, W, with_n, S):
    rng = np.random.default_rng(100 * W + 10 * S + with_n)
    hi = {1: 32, 2: 64, 8: 255}[W]
    seqs = model.random_reads(rng, 600, lo=1, hi=hi, p_n=0.05 if with_n else 0.0)
    seqs[:40] = model.random_reads(rng, 40, lo=hi, hi=hi, p_n=0.05 if with_n else 0.0)   # (the last base of the last word)
    seqs = list(dict.fromkeys(seqs))
    words, lens, nmask = pack.pack_reads(seqs, W)
    assert words.shape[0] == W and (nmask is not None) == with_n
    quant = zipf_quant(rng, len(seqs), S)
    quant[:50] = 3                                                        # (ties in every column: the string decides)
    samples = ["s%d.fastq" % i for i in range(S)]
    host, arrays = tmp_path / "host", tmp_path / "arrays"
    host.mkdir()
    arrays.mkdir()
    report.write_collapsed_fa_host(str(host), samples, words, lens, nmask, quant, {})
    orders = [model.order(seqs, quant[:, s]) for s in range(S)]
    rows = columnar.write_collapsed_fa(str(arrays), samples, words, lens, nmask, quant, orders, {})
    for s in range(S):
        fn = "s%d.trim.collapse.fa" % s
        got = (arrays / fn).read_bytes()
        assert got == (host / fn).read_bytes() == model.text(seqs, quant[:, s]), fn
        assert rows[s] == int(np.count_nonzero(quant[:, s])) == got.count(b">")


def test_a_sample_without_reads_gives_an_empty_file(native_lib, tmp_path):
    seqs = ["ACGTACGTACGTACGTA", "TTTTACGTACGTACGTAN"]
    words, lens, nmask = pack.pack_reads(seqs)
    quant = np.array([[5, 0], [2, 0]], dtype=np.uint32)
    rows = columnar.write_collapsed_fa(str(tmp_path), ["a.fq", "b.fq"], words, lens, nmask, quant,
                                       [model.order(seqs, quant[:, 0]), np.zeros(0, np.uint32)], {})
    assert rows == [2, 0]
    assert (tmp_path / "b.trim.collapse.fa").read_bytes() == b""
    assert (tmp_path / "a.trim.collapse.fa").read_bytes() == model.text(seqs, quant[:, 0])
    # no reads at all
    empty = np.zeros((1, 0), np.uint64), np.zeros(0, np.uint8), None, np.zeros((0, 1), np.uint32)
    assert columnar.write_collapsed_fa(str(tmp_path), ["c.fq"], *empty, [np.zeros(0, np.uint32)], {}) == [0]
    assert (tmp_path / "c.trim.collapse.fa").read_bytes() == b""


def test_reads_beyond_255_nt_merge_in_by_count_and_string(native_lib, tmp_path):
    rng = np.random.default_rng(7)
    seqs = ["C" + s for s in model.random_reads(rng, 200, lo=16, hi=200, p_n=0.03)] + ["G" + "ACGT" * 5, "G" + "ACGT" * 4]
    words, lens, nmask = pack.pack_reads(seqs)
    quant = np.zeros((len(seqs), 2), dtype=np.uint32)
    quant[:, 0] = rng.integers(10, 50, len(seqs))
    quant[:60, 0] = 9                                   # the packed reads the first two extra rows tie with
    quant[:, 1] = rng.integers(0, 3, len(seqs))
    tail = "ACGT" * 70
    long_counts = {
        "T" + tail: [9, 1],                             # ties with packed reads, above every one of them as a string
        "A" + tail: [9, 0],                             # ties with packed reads, below every one of them
        "G" + "ACGT" * 5 + tail: [9, 0],                # ... and between two of them, a packed read its proper prefix
        "CC" + tail: [1000, 2],                         # the top count
        "GG" + tail: [1, 7],                            # the lowest count (sample 0), the top count (sample 1)
        "NN" + tail: [0, 1],                            # no count in sample 0
    }
    quant[-2:, 0] = 9
    samples = ["x.fastq", "y.fastq"]
    host, arrays = tmp_path / "host", tmp_path / "arrays"
    host.mkdir()
    arrays.mkdir()
    report.write_collapsed_fa_host(str(host), samples, words, lens, nmask, quant, long_counts)
    orders = [model.order(seqs, quant[:, s]) for s in range(2)]
    rows = columnar.write_collapsed_fa(str(arrays), samples, words, lens, nmask, quant, orders, long_counts)
    for s, fn in enumerate(("x.trim.collapse.fa", "y.trim.collapse.fa")):
        extra = [(k, v[s]) for k, v in long_counts.items()]
        got = (arrays / fn).read_bytes()
        assert got == (host / fn).read_bytes() == model.text(seqs, quant[:, s], extra), fn
        assert rows[s] == got.count(b">")
    lines = (arrays / "x.trim.collapse.fa").read_text().split("\n")
    assert lines[0] == ">seq1_1000" and lines[1] == "CC" + tail and lines[-3] == ">seq%d_1" % rows[0] and lines[-2] == "GG" + tail
    nine = [lines[i + 1] for i in range(0, len(lines) - 1, 2) if lines[i].endswith("_9")]
    assert nine[0] == "T" + tail and nine[-1] == "A" + tail and len(nine) == 65
    at = nine.index("G" + "ACGT" * 5 + tail)
    assert nine[at + 1] == "G" + "ACGT" * 5 and nine[at + 2] == "G" + "ACGT" * 4


def test_device_entry_points_check_their_arguments_without_a_gpu(native_lib):
    L = native_lib
    a, b = C.c_uint64(), C.c_uint64()
    assert L.mrg_collapsed_order_temp_bytes(1000, None, C.byref(b)) < 0 and b"null" in L.mrg_last_error()
    assert L.mrg_collapsed_order_temp_bytes(1000, C.byref(a), None) < 0
    assert L.mrg_collapsed_order_temp_bytes(2 ** 31, C.byref(a), C.byref(b)) < 0
    for n in (1, 1000, 65537):
        assert L.mrg_collapsed_order_temp_bytes(n, C.byref(a), C.byref(b)) == 0
        assert a.value >= 24 * n and b.value >= a.value + 4 * (n + 1)      # two key and two value buffers; the flags
    rows = C.c_uint64()
    assert L.mrg_seq_rank(None, None, 1, 0, None, None, 0, 0, None, None, 0, None) < 0 and b"mrg_seq_rank: null" in L.mrg_last_error()
    assert L.mrg_collapsed_order(None, None, 0, 0, 0, None, None, 0, C.byref(rows), None, 0, None) < 0
    assert b"mrg_collapsed_order: null" in L.mrg_last_error()


def test_error_paths_write_nothing(native_lib, tmp_path):
    L = native_lib
    seqs = ["ACGTACGTACGTACGTA", "TTTTACGTACGTACGTAC", "GGGGACGTACGTACGTAC"]
    words, lens, nmask = pack.pack_reads(seqs)
    quant = np.array([[5, 0], [2, 1], [0, 4]], dtype=np.uint32)
    path = str(tmp_path / "out.fa")
    x = words.ctypes.data

    def refused(rc, word):
        assert rc < 0 and word in L.mrg_last_error(), (rc, L.mrg_last_error())
        assert not os.path.exists(path)
    good = np.array([0, 1], dtype=np.uint32)
    assert native_write(L, path, words, lens, nmask, quant, 0, good) == 2
    assert open(path, "rb").read() == model.text(seqs, quant[:, 0])
    os.remove(path)
    refused(L.mrg_write_collapsed_fasta(None, x, 1, 3, x, None, 3, x, 2, 0, x, 2, None, None, 0), b"null")
    for hole in range(4):   # reads, lens, quant, order
        a = [x, x, x, x]
        a[hole] = None
        refused(L.mrg_write_collapsed_fasta(os.fsencode(path), a[0], 1, 3, a[1], None, 3, a[2], 2, 0, a[3], 2, None, None, 0), b"null")
    refused(L.mrg_write_collapsed_fasta(os.fsencode(path), x, 1, 3, x, None, 3, x, 2, 0, x, 2, None, None, 1), b"null")
    refused(L.mrg_write_collapsed_fasta(os.fsencode(path), x, 3, 3, x, None, 3, x, 2, 0, x, 2, None, None, 0), b"words_per_read")
    refused(L.mrg_write_collapsed_fasta(os.fsencode(path), x, 1, 2, x, None, 3, x, 2, 0, x, 2, None, None, 0), b"stride")
    refused(native_write(L, path, words, lens, nmask, quant, 2, good), b"sample 2 of 2")
    refused(native_write(L, path, words, lens, nmask, quant, 0, np.array([0, 3], np.uint32)), b"order[1] = 3 is no read")
    refused(native_write(L, path, words, lens, nmask, quant, 0, np.array([0, 1, 2], np.uint32)), b"read 2 has no count")
    refused(native_write(L, path, words, lens, nmask, quant, 0, np.array([0xFFFFFFFF], np.uint32)), b"is no read")
    tail = "ACGT" * 70
    refused(native_write(L, path, words, lens, nmask, quant, 0, good, [("A" + tail, 3), ("C" + tail, 3)]), b"descending")
    refused(native_write(L, path, words, lens, nmask, quant, 0, good, [("A" + tail, 3), ("A" + tail, 4)]), b"descending")
    refused(native_write(L, path, words, lens, nmask, quant, 0, good, [("A" + tail, 0)]), b"no count")
    # a bad order met after good rows: still nothing on disk, and an earlier file is left as it was
    assert native_write(L, path, words, lens, nmask, quant, 1, np.array([2, 1], np.uint32)) == 2
    before = open(path, "rb").read()
    assert native_write(L, path, words, lens, nmask, quant, 1, np.array([2, 1, 0], np.uint32)) < 0
    assert open(path, "rb").read() == before == model.text(seqs, quant[:, 1])
    # the Python wrapper raises
    from mirge_amd._native import MirgeAmdError
    with pytest.raises(MirgeAmdError):
        columnar.write_collapsed_fa(str(tmp_path), ["z.fq"], words, lens, nmask, quant[:, :1], [np.array([2], np.uint32)], {})
    assert not os.path.exists(str(tmp_path / "z.trim.collapse.fa"))
    # an unwritable path is an I/O error
    assert native_write(L, str(tmp_path / "no" / "dir.fa"), words, lens, nmask, quant, 0, good) < 0
    assert b"cannot open" in L.mrg_last_error()
