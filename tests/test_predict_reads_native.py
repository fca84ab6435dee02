"""Predict mode's candidate reads on the host: the model (tests/predict_reads_model.py) against the files the reference's
convert2Fasta wrote (tests/golden/predict_reads.json), the native writer and the name builder (mrg_write_predict_fasta,
mrg_predict_read_names; predict.write_candidate_reads / read_names) against the model's text, the error paths, the
argument checks of the device entry points, and the command line's new options."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from mirge_amd import pack, predict
from tests import predict_reads_model as model
from tests.conftest import ROOT


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "predict_reads.json")) as fh:
        return json.load(fh)["cases"]


def model_lists(seqs, quant, min_len, max_len, cutoff, unmapped=None, S=None):
    """The dict predict.candidate_lists returns, from the model (host arrays)."""
    n = len(seqs)
    S = len(quant[0]) if S is None else S
    um = [True] * n if unmapped is None else unmapped
    total, raw_no, sel_no, n_raw, n_sel = model.select([len(s) for s in seqs], um, quant, min_len, max_len, cutoff)

    def rows(triples, dt):
        return (np.array([t[0] for t in triples], np.uint32), np.array([t[1] for t in triples], np.uint32),
                np.array([t[2] for t in triples], dt))
    out = dict(n_raw=n_raw, n_sel=n_sel,
               raw=rows([(u, no, total[u]) for u, no in enumerate(raw_no) if no], np.uint64),
               sel=rows([(u, no, total[u]) for u, no in enumerate(sel_no) if no], np.uint64))
    out["sample_raw"] = [rows(model.sample_rows(raw_no, quant, s, 1), np.uint32) for s in range(S)]
    out["sample_sel"] = [rows(model.sample_rows(sel_no, quant, s, cutoff), np.uint32) for s in range(S)]
    return out


def read_dir(path):
    return {fn: open(os.path.join(path, fn)).read() for fn in sorted(os.listdir(path))}


def test_the_fixture_covers_the_cases_of_the_contract(golden):
    names = {c["name"] for c in golden}
    assert {"one_stem", "one_stem_of_three", "empty"} <= names and len(golden) == 27
    assert {(c["min_len"], c["max_len"], c["cutoff"]) for c in golden} >= {(16, 25, 1), (16, 25, 2), (16, 25, 5), (20, 20, 2)}
    assert {c["spike"] for c in golden} == {False, True}
    lens, sizes = set(), set()
    for c in golden:
        samples, seqs, quant = model.from_csv(c["csv"], c["spike"])
        sizes.add(len(samples))
        lens |= {len(s) for s in seqs}
        assert len(c["files"]) == 2 + 2 * len({model.stem(s) for s in samples})
    assert sizes == {1, 2, 3} and {15, 16, 25, 26} <= lens
    c = next(c for c in golden if c["name"] == "S2_spike0_16_25_2")
    samples, seqs, quant = model.from_csv(c["csv"])
    assert quant[5] == [1, 1] and len(seqs[5]) in range(16, 26)      # the sum reaches the cutoff, no sample does
    assert ("\n" + seqs[5] + "\n") in c["files"]["unmapped_mirna.fa"]
    assert all(seqs[5] not in c["files"]["unmapped_mirna_s%d.fa" % k] for k in range(2))
    assert any("N" in s for s in seqs) and any(sum(q) == 0 for q in quant)
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "predict_reads.json")) < 200_000


def test_model_reproduces_the_reference_files(golden):
    for c in golden:
        samples, seqs, quant = model.from_csv(c["csv"], c["spike"])
        assert model.csv_text(samples, seqs, quant, c["spike"]) == c["csv"], c["name"]
        assert model.files(samples, seqs, quant, c["min_len"], c["max_len"], c["cutoff"]) == c["files"], c["name"]


@pytest.mark.parametrize("threads", [1, 16])
def test_native_writer_reproduces_the_reference_files(native_lib, golden, tmp_path, monkeypatch, threads):
    monkeypatch.setenv("MIRGE_AMD_TABLE_THREADS", str(threads))
    monkeypatch.setenv("MIRGE_AMD_PREDICT_BLOCK_ROWS", "3")
    for c in golden:
        samples, seqs, quant = model.from_csv(c["csv"], c["spike"])
        words, lens, nmask = pack.pack_reads(seqs) if seqs else (np.zeros((1, 0), np.uint64), np.zeros(0, np.uint8), None)
        out = tmp_path / ("%s_%d" % (c["name"], threads))
        out.mkdir()
        lists = model_lists(seqs, quant, c["min_len"], c["max_len"], c["cutoff"], S=len(samples))
        rows = predict.write_candidate_reads(str(out), samples, words, lens, nmask, lists, c["min_len"], c["max_len"], c["cutoff"])
        got = read_dir(str(out))
        assert got == c["files"], c["name"]
        assert {fn: t.count(">") for fn, t in got.items()} == rows


@pytest.mark.parametrize("W", [1, 2, 8])
def test_native_writer_on_wide_reads_mapped_reads_and_long_reads(native_lib, tmp_path, W):
    """Reads up to the last base of the last word, mapped reads among them (not listed, their numbers skipped), and reads
    beyond 255 nt at the end of the table: in the raw files always, in the filtered files when the window admits them."""
    rng = np.random.default_rng(W)
    hi = {1: 32, 2: 64, 8: 255}[W]
    seqs = model.random_reads(rng, 300, [16, 20, 25, hi - 1, hi], p_n=0.03)
    words, lens, nmask = pack.pack_reads(seqs, W)
    quant = rng.choice([0, 1, 2, 7, 300], size=(len(seqs), 2)).tolist()
    unmapped = (rng.random(len(seqs)) < 0.7).tolist()
    tail = "ACGT" * 70
    long_rows = [("T" + tail, [3, 0]), ("NA" + tail, [0, 0]), ("G" + tail, [1, 1]), ("C" + tail, [0, 9])]
    samples = ["left.fastq", "right.fq"]
    for max_len in (hi, 400):
        lists = model_lists(seqs, quant, 16, max_len, 2, unmapped)
        out = tmp_path / ("out%d" % max_len)
        out.mkdir()
        predict.write_candidate_reads(str(out), samples, words, lens, nmask, lists, 16, max_len, 2, long_rows)
        all_seqs, all_quant = seqs + [r[0] for r in long_rows], quant + [r[1] for r in long_rows]
        want = model.files(samples, all_seqs, all_quant, 16, max_len, 2, unmapped + [True] * len(long_rows))
        assert read_dir(str(out)) == want
        raw = want["unmapped_mirna_raw.fa"].split("\n")
        assert raw[-2] == "C" + tail and raw[-3] == ">mir%d_9" % (lists["n_raw"] + 3)
        assert (("G" + tail) in want["unmapped_mirna.fa"]) == (max_len == 400)
        assert ("G" + tail) not in want["unmapped_mirna_left.fa"] and ("T" + tail in want["unmapped_mirna_left.fa"]) == (max_len == 400)


def test_totals_of_two_to_the_32_and_above(native_lib, tmp_path):
    seqs = ["ACGTACGTACGTACGTAC", "TTTTACGTACGTACGTACGT", "GGGGACGTACGTACGTACN"]
    words, lens, nmask = pack.pack_reads(seqs)
    quant = [[2 ** 31, 2 ** 31], [2 ** 32 - 1, 2 ** 32 - 1], [2 ** 32 - 1, 0]]
    lists = model_lists(seqs, quant, 16, 25, 2)
    assert lists["sel"][2].dtype == np.uint64 and lists["sel"][2].tolist() == [2 ** 32, 2 ** 33 - 2, 2 ** 32 - 1]
    predict.write_candidate_reads(str(tmp_path), ["a.fq", "b.fq"], words, lens, nmask, lists, 16, 25, 2)
    got = read_dir(str(tmp_path))
    assert got == model.files(["a.fq", "b.fq"], seqs, quant, 16, 25, 2)
    assert got["unmapped_mirna.fa"].startswith(">mir1_4294967296\nACGTACGTACGTACGTAC\n>mir2_8589934590\n")
    assert got["unmapped_mirna_a.fa"].startswith(">mir1_2147483648\n") and ">mir3_4294967295\n" in got["unmapped_mirna_a_raw.fa"]


def native_write(lib, path, words, lens, nmask, idx, num, cnt, extra=()):
    words = np.ascontiguousarray(words, dtype=np.uint64)
    W, n = words.shape
    idx, num = np.ascontiguousarray(idx, dtype=np.uint32), np.ascontiguousarray(num, dtype=np.uint32)
    cnt = np.ascontiguousarray(cnt)
    seqs = (C.c_char_p * max(len(extra), 1))(*[e[0].encode() for e in extra])
    e_num = np.array([e[1] for e in extra], dtype=np.uint64)
    e_cnt = np.array([e[2] for e in extra], dtype=np.uint64)
    return lib.mrg_write_predict_fasta(os.fsencode(path), words.ctypes.data, W, n, lens.ctypes.data,
                                       None if nmask is None else nmask.ctypes.data, n, idx.ctypes.data, num.ctypes.data,
                                       cnt.ctypes.data, cnt.dtype.itemsize, idx.shape[0], seqs, e_num.ctypes.data, e_cnt.ctypes.data,
                                       len(extra))


def test_error_paths_write_nothing(native_lib, tmp_path):
    L = native_lib
    seqs = ["ACGTACGTACGTACGTA", "TTTTACGTACGTACGTAC", "GGGGACGTACGTACGTAC"]
    words, lens, nmask = pack.pack_reads(seqs)
    path = str(tmp_path / "out.fa")
    x = words.ctypes.data
    u32 = lambda *v: np.array(v, dtype=np.uint32)
    tail = "ACGT" * 70

    def refused(rc, word):
        assert rc < 0 and word in L.mrg_last_error(), (rc, L.mrg_last_error())
        assert not os.path.exists(path)
    assert native_write(L, path, words, lens, nmask, u32(0, 2), u32(1, 2), u32(5, 6), [(tail, 3, 2 ** 40)]) == 3
    assert open(path).read() == ">mir1_5\n%s\n>mir2_6\n%s\n>mir3_%d\n%s\n" % (seqs[0], seqs[2], 2 ** 40, tail)
    os.remove(path)
    assert native_write(L, path, words, lens, nmask, u32(), u32(), u32()) == 0 and open(path).read() == ""      # k = 0
    os.remove(path)
    refused(L.mrg_write_predict_fasta(None, x, 1, 3, x, None, 3, x, x, x, 4, 2, None, None, None, 0), b"null")
    for hole in range(5):   # reads, lens, idx, num, counts
        a = [x] * 5
        a[hole] = None
        refused(L.mrg_write_predict_fasta(os.fsencode(path), a[0], 1, 3, a[1], None, 3, a[2], a[3], a[4], 4, 2, None, None, None, 0),
                b"null")
    refused(L.mrg_write_predict_fasta(os.fsencode(path), x, 1, 3, x, None, 3, x, x, x, 4, 2, None, None, None, 1), b"null extra")
    refused(L.mrg_write_predict_fasta(os.fsencode(path), x, 3, 3, x, None, 3, x, x, x, 4, 2, None, None, None, 0), b"words_per_read")
    refused(L.mrg_write_predict_fasta(os.fsencode(path), x, 1, 2, x, None, 3, x, x, x, 4, 2, None, None, None, 0), b"stride")
    refused(L.mrg_write_predict_fasta(os.fsencode(path), x, 1, 3, x, None, 3, x, x, x, 2, 2, None, None, None, 0), b"count_bytes")
    refused(native_write(L, path, words, lens, nmask, u32(0, 3), u32(1, 2), u32(5, 6)), b"index[1] = 3 is no read")
    refused(native_write(L, path, words, lens, nmask, u32(0xFFFFFFFF), u32(1), u32(5)), b"is no read")
    refused(native_write(L, path, words, lens, nmask, u32(0, 1), u32(0, 1), u32(5, 6)), b"number 0")
    refused(native_write(L, path, words, lens, nmask, u32(0, 1), u32(1, 0), u32(5, 6)), b"number 0")
    refused(native_write(L, path, words, lens, nmask, u32(0, 1), u32(2, 2), u32(5, 6)), b"do not increase")
    refused(native_write(L, path, words, lens, nmask, u32(0, 1, 2), u32(1, 3, 2), u32(5, 6, 7)), b"do not increase")
    refused(native_write(L, path, words, lens, nmask, u32(1, 0), u32(1, 2), u32(5, 6)), b"indices")
    refused(native_write(L, path, words, lens, nmask, u32(0, 1), u32(1, 2), u32(5, 6), [(tail, 2, 1)]), b"extra row 0 does not increase")
    refused(native_write(L, path, words, lens, nmask, u32(0), u32(1), u32(5), [(tail, 3, 1), (tail, 3, 1)]), b"extra row 1 does not increase")
    refused(native_write(L, path, words, lens, nmask, u32(), u32(), u32(), [(tail, 0, 1)]), b"number 0")
    # a bad row met after good ones: still nothing on disk, and an earlier file is left as it was
    assert native_write(L, path, words, lens, nmask, u32(1), u32(4), u32(9)) == 1
    before = open(path).read()
    assert native_write(L, path, words, lens, nmask, u32(0, 1, 7), u32(1, 2, 3), u32(5, 6, 7)) < 0
    assert open(path).read() == before == ">mir4_9\n%s\n" % seqs[1]
    # the Python wrapper raises
    from mirge_amd._native import MirgeAmdError
    lists = model_lists(seqs, [[3], [3], [3]], 16, 25, 2)
    lists["sel"] = (u32(0, 5), u32(1, 2), np.array([3, 3], np.uint64))
    with pytest.raises(MirgeAmdError):
        predict.write_candidate_reads(str(tmp_path), ["z.fq"], words, lens, nmask, lists, 16, 25, 2)
    assert not os.path.exists(str(tmp_path / "unmapped_mirna.fa"))
    # an unwritable path is an I/O error
    assert native_write(L, str(tmp_path / "no" / "dir.fa"), words, lens, nmask, u32(0), u32(1), u32(5)) < 0
    assert b"cannot open" in L.mrg_last_error()


def test_read_names(native_lib):
    rng = np.random.default_rng(3)
    num = np.sort(rng.choice(10 ** 7, 5000, replace=False)).astype(np.uint32) + 1
    for dt, top in ((np.uint32, 2 ** 32), (np.uint64, 2 ** 40)):
        cnt = rng.integers(0, top, 5000).astype(dt)
        cnt[:3] = [0, 1, top - 1] if dt == np.uint32 else [2 ** 32, 2 ** 33, 2 ** 64 - 1]
        blob, off = predict.read_names(num, cnt)
        want = ["mir%d_%d" % (a, b) for a, b in zip(num.tolist(), cnt.tolist())]
        assert blob == "".join(want).encode() and off.dtype == np.uint64
        assert off.tolist() == np.concatenate([[0], np.cumsum([len(w) for w in want])]).tolist()
        if dt == np.uint32:
            assert predict.read_counts(want).tolist() == cnt.tolist()
    blob, off = predict.read_names(np.zeros(0, np.uint32), np.zeros(0, np.uint32))
    assert blob == b"" and off.tolist() == [0]
    L = native_lib
    need, offs = C.c_uint64(), (C.c_uint64 * 3)()
    a = np.array([1, 2], np.uint32)
    assert L.mrg_predict_read_names(a.ctypes.data, a.ctypes.data, 4, 2, None, 0, None, C.byref(need)) < 0 and b"null" in L.mrg_last_error()
    assert L.mrg_predict_read_names(a.ctypes.data, a.ctypes.data, 4, 2, None, 0, offs, None) < 0
    assert L.mrg_predict_read_names(None, a.ctypes.data, 4, 2, None, 0, offs, C.byref(need)) < 0
    assert L.mrg_predict_read_names(a.ctypes.data, a.ctypes.data, 3, 2, None, 0, offs, C.byref(need)) < 0 and b"count_bytes" in L.mrg_last_error()
    small = C.create_string_buffer(5)
    assert L.mrg_predict_read_names(a.ctypes.data, a.ctypes.data, 4, 2, small, 5, offs, C.byref(need)) < 0 and need.value == 12
    assert b"do not fit" in L.mrg_last_error()


def test_writers_take_a_blob_pair_for_names_and_sequences(native_lib, tmp_path):
    """predict.write_clusters / write_sorted_sam: a ready (blob, offsets) pair gives the bytes a list gives."""
    from mirge_amd.index import FmIndex
    rng = np.random.default_rng(5)
    chrom = "".join("ACGT"[c] for c in rng.integers(0, 4, 300))
    parts = [FmIndex.build(["chr1"], [chrom])]
    seqs = [chrom[10:32], chrom[14:36], "ACGTNACGTACGTACGTACGT"]
    num, cnt = np.array([1, 4, 9], np.uint32), np.array([7, 2, 3], np.uint32)
    names = ["mir%d_%d" % (a, b) for a, b in zip(num, cnt)]
    words, lens, nmask = pack.pack_reads(seqs)
    pair_names, pair_seqs = predict.read_names(num, cnt), pack.unpack_blob(words, lens, nmask)
    assert pair_seqs[0] == "".join(seqs).encode() and pair_seqs[1].tolist() == [0, 22, 44, 65]
    rows = (np.array([0, 1], np.uint32), np.array([0, 0], np.int32), np.array([10, 14], np.int32), np.zeros(2, np.uint8),
            np.zeros(2, np.uint8))
    supp = np.zeros(3, bool)
    a = predict.write_sorted_sam(str(tmp_path / "list.sam"), parts, names, seqs, rows, supp, 3)
    b = predict.write_sorted_sam(str(tmp_path / "pair.sam"), parts, pair_names, pair_seqs, rows, supp, 3)
    text = (tmp_path / "pair.sam").read_bytes()
    assert a == b and text == (tmp_path / "list.sam").read_bytes()
    assert b"mir1_7\t0\tchr1\t11\t" in text and b"mir9_3\t4\t" in text
    cl = dict(entry=np.zeros(1, np.uint32), strand=np.zeros(1, np.uint8), start=np.array([11], np.uint32), end=np.array([36], np.uint32),
              seq_off=np.array([0, 26], np.uint64), seq=chrom[10:36].encode(), count_sum=np.array([9], np.uint64),
              member_off=np.array([0, 2], np.uint32), members=np.array([0, 1], np.uint32))
    assert predict.write_clusters(str(tmp_path / "list.tsv"), "s", parts, names, cl) == 1
    assert predict.write_clusters(str(tmp_path / "pair.tsv"), "s", parts, pair_names, cl) == 1
    text = (tmp_path / "pair.tsv").read_bytes()
    assert text == (tmp_path / "list.tsv").read_bytes() and b"mir1_7,mir4_2" in text
    with pytest.raises(ValueError):
        predict.write_sorted_sam(str(tmp_path / "bad.sam"), parts, pair_names, seqs[:2], rows, supp, 3)
    # a tuple of names is a sequence of names, also when it has two of them
    predict.write_sorted_sam(str(tmp_path / "tuple.sam"), parts, tuple(names), tuple(seqs), rows, supp, 3)
    assert (tmp_path / "tuple.sam").read_bytes() == (tmp_path / "list.sam").read_bytes()
    two = (np.array([0, 1], np.uint32),) + tuple(a[:2] for a in rows[1:])
    a = predict.write_sorted_sam(str(tmp_path / "two_list.sam"), parts, names[:2], seqs[:2], two, supp[:2], 3)
    b = predict.write_sorted_sam(str(tmp_path / "two_tuple.sam"), parts, tuple(names[:2]), tuple(seqs[:2]), two, supp[:2], 3)
    assert a == b and (tmp_path / "two_tuple.sam").read_bytes() == (tmp_path / "two_list.sam").read_bytes()


def test_device_entry_points_check_their_arguments_without_a_gpu(native_lib):
    L = native_lib
    b = C.c_uint64()
    assert L.mrg_predict_reads_temp_bytes(1000, None) < 0 and b"null" in L.mrg_last_error()
    assert L.mrg_predict_reads_temp_bytes(2 ** 31, C.byref(b)) < 0 and b"limit" in L.mrg_last_error()
    for n in (0, 1, 1000, 65537):
        assert L.mrg_predict_reads_temp_bytes(n, C.byref(b)) == 0 and b.value >= 8 * (n + 1) + 16      # two flag arrays; the stat words
    r0, r1 = C.c_uint64(7), C.c_uint64(7)
    assert L.mrg_predict_select(None, None, None, None, 0, 1, 16, 25, 2, None, None, None, C.byref(r0), C.byref(r1), None, 0, None) < 0
    assert b"mrg_predict_select: null" in L.mrg_last_error()
    assert L.mrg_predict_sample_reads(None, None, 0, 1, 0, None, 1, None, None, None, 0, C.byref(r0), None, 0, None) < 0
    assert b"mrg_predict_sample_reads: null" in L.mrg_last_error()
    assert L.mrg_predict_gather(None, None, 1, 0, None, None, 0, None, 1, 0, None, 0, None, None, None, None, None, 0, None) < 0
    assert b"mrg_predict_gather: null" in L.mrg_last_error()


def test_no_device_is_reported_not_a_crash(native_lib):
    """Exercises context creation only, which is behaviour from before these calls (it passes without them): the new device
    calls need a context, and without a device its creation says MRG_ERR_NO_DEVICE, so Engine.predict_select is never
    reached and nothing runs.  With a device there is nothing to check here."""
    import torch
    from mirge_amd import _native
    if torch.cuda.is_available():
        return
    h = C.c_void_p()
    assert L_create(native_lib, h) == _native.MRG_ERR_NO_DEVICE and not h.value
    from mirge_amd.engine import Engine
    with pytest.raises(_native.MirgeAmdError) as ei:
        Engine(0).predict_select(np.zeros(1, np.int8), np.zeros(1, np.uint8), np.zeros((1, 1), np.uint32))
    assert ei.value.code == _native.MRG_ERR_NO_DEVICE


def L_create(lib, handle):
    return lib.mrg_ctx_create(0, C.byref(handle))


def test_parser_takes_the_new_options():
    from mirge_amd import cli
    base = ["annotate", "-s", "a.fastq", "-lib", "/L", "-sp", "human"]
    a = cli.build_parser().parse_args(base)
    assert not a.novel_reads and not a.novel_clusters
    assert (a.minLength, a.maxLength, a.countCutoff) == ("16", "25", "2")          # parseArgument.py:86-88: strings
    assert (a.mapping_loc, a.seedLength, a.overlapLenCutoff) == ("3", "25", "14")  # :89-91
    a = cli.build_parser().parse_args(base + ["--novel-clusters", "-minl", "18", "-maxl", "30", "-cc", "5", "-ml", "2", "-sl", "20",
                                              "-olc", "10"])
    assert a.novel_clusters and not a.novel_reads
    assert (a.minLength, a.maxLength, a.countCutoff, a.mapping_loc, a.seedLength, a.overlapLenCutoff) == ("18", "30", "5", "2", "20", "10")
    assert cli.build_parser().parse_args(base + ["--novel-reads"]).novel_reads
