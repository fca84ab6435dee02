"""GPU (-m gpu): mrg_isomir_classify (csrc/isomir_gff.hip) called directly with hand-made pass_id / ref_id / pos
arrays, against isomir.classify_alignment through tests/isomir_rows_model.py; then Engine.isomir_classify +
columnar.write_isomir_gff on the golden alignments and `annotate -gff` with and without --gff-host.  Everything is
compared for equality; there is no tolerance anywhere.

Every output buffer carries GUARD rows of a byte pattern behind the capacity, which must come back untouched.

The issue's list of first-mismatch classes names x - frame0 in {0, 1, ...}: those two cannot occur (frame0 <= m0 - 2 and
the overlap starts at x >= m0, so x - frame0 >= 2; classify_alignment cannot return them either).  The enumeration walks
EVERY mismatch position of the overlap, so every reachable value, 2 .. 24 and beyond, is covered."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from mirge_amd import isomir, pack
from tests import isomir_rows_model as model
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu

GUARD = 16
PAT = 0xA5


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "isomir_gff.json")) as fh:
        return json.load(fh)


class Gpu:
    def __init__(self):
        import torch
        from mirge_amd.engine import Engine
        self.torch = torch
        self.eng = Engine(0)
        self.lib = self.eng._lib
        self.dev = self.eng.device

    def up(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)

    def classify(self, table, words, lens, nmask, pass_id, ref_id, pos, cap=None, pad=0, canon=0, iso=8):
        """-> (idx, rec, mask, n_canon, n_isomir) of the rows below the capacity (default: all of them); the guards
        behind the capacity are checked.  pad: extra columns of junk behind the reads (stride = n + pad)."""
        W, n = words.shape
        if pad:
            junk = np.full((W, pad), 0xDEADBEEFDEADBEEF, dtype=np.uint64)
            words = np.concatenate([words, junk], axis=1)
            nmask = None if nmask is None else np.concatenate([nmask, junk], axis=1)
        d_words = self.up(words.view(np.int64))
        d_nmask = None if nmask is None else self.up(nmask.view(np.int64))
        d_lens, d_pass = self.up(np.asarray(lens, dtype=np.uint8)), self.up(np.asarray(pass_id, dtype=np.int8))
        d_ref, d_pos = self.up(np.asarray(ref_id, dtype=np.int32)), self.up(np.asarray(pos, dtype=np.int32))
        desc = np.ascontiguousarray(table.desc, dtype=np.int32)
        counts = (C.c_uint64 * 2)()
        stream = self.eng._stream_ptr()

        def call(c, idx, rec, mask):
            rc = self.lib.mrg_isomir_classify(
                self.eng._h, d_words.data_ptr(), W, n + pad, d_lens.data_ptr(), None if d_nmask is None else d_nmask.data_ptr(),
                n, d_pass.data_ptr(), d_ref.data_ptr(), d_pos.data_ptr(), canon, iso, desc.ctypes.data, desc.shape[0],
                table.words.ctypes.data, table.nplane.ctypes.data, table.words.shape[0], c,
                None if idx is None else idx.data_ptr(), None if rec is None else rec.data_ptr(),
                None if mask is None else mask.data_ptr(), counts, None, stream)
            assert rc == 0, self.lib.mrg_last_error()
        call(0, None, None, None)
        k = int(counts[0]) + int(counts[1])
        first = (int(counts[0]), int(counts[1]))
        cap = k if cap is None else cap
        mw = model.mask_words(W)
        bufs = [self.torch.full(((cap + GUARD) * width,), PAT, dtype=self.torch.uint8, device=self.dev)
                for width in (4, 32, 8 * mw)]
        call(cap, *bufs)
        assert (int(counts[0]), int(counts[1])) == first, "the counts of the filling call differ from the counting call's"
        rows = min(k, cap)
        out = []
        for buf, width, dtype in zip(bufs, (4, 32, 8 * mw), (np.uint32, np.int32, np.uint64)):
            raw = buf.cpu().numpy()
            assert (raw[rows * width:] == PAT).all(), "written behind row %d (capacity %d, %d selected)" % (rows, cap, k)
            out.append(raw[:rows * width].view(dtype))
        return out[0], out[1].reshape(rows, 8), out[2].reshape(rows, mw), first[0], first[1]


@pytest.fixture(scope="module")
def gpu():
    return Gpu()


def case_table(cases):
    """Every case (P, E, R, start, index_value) is its own library entry with its own precursor."""
    names = ["c%d" % i for i in range(len(cases))]
    hairpin = {"c%d_pre" % i: c[0] for i, c in enumerate(cases)}
    return isomir.entry_table(names, [c[1] for c in cases], hairpin, {}, "MirGeneDB")


def run_cases(gpu, cases, W, decode_all=False):
    """The cases through the kernel with W words per read: records and masks equal the model's; decoded, they equal
    classify_alignment's answers.  Returns the decoded results in case order."""
    table = case_table(cases)
    assert not table.errors
    n = len(cases)
    words, lens, nmask = pack.pack_reads([c[2] for c in cases], W)
    pass_id = np.array([0 if c[4] == 0 else 8 for c in cases], dtype=np.int8)
    idx, rec, mask, n_canon, n_iso = gpu.classify(table, words, lens, nmask, pass_id, np.arange(n), [c[3] - 1 for c in cases])
    assert (n_canon, n_iso) == (int((pass_id == 0).sum()), int((pass_id == 8).sum()))
    assert np.array_equal(idx, np.concatenate([np.nonzero(pass_id == 0)[0], np.nonzero(pass_id == 8)[0]]))
    got = [None] * n
    mw = model.mask_words(W)
    for row, i in enumerate(idx.tolist()):
        P, E, R, start, iv = cases[i]
        want_rec, want_mask = model.encode(P, E, R, start, iv, i, 8)
        assert not want_mask[mw:].any()
        if not (np.array_equal(rec[row], want_rec) and np.array_equal(mask[row], want_mask[:mw])):
            raise AssertionError("case %r (W = %d): record %s mask %s, model %s %s" % (
                cases[i], W, rec[row].tolist(), [hex(int(x)) for x in mask[row]], want_rec.tolist(),
                [hex(int(x)) for x in want_mask[:mw]]))
        if decode_all:
            got[i] = model.decode(rec[row], mask[row], R)
            assert got[i] == isomir.classify_alignment(P, E, R, start, iv), cases[i]
    return got


def test_the_700_reference_cases(gpu, golden):
    raw = golden["expected"]["classify"]
    cases = [tuple(c[:5]) for c in raw]
    got = run_cases(gpu, cases, 1, decode_all=True)
    dropped = 0
    for c, g in zip(raw, got):
        assert (None if g is None else list(g)) == c[5], c[:5]
        dropped += g is None
    assert dropped == 23 and len(cases) == 700


def rnd_seq(rng, n, alphabet="ACGT"):
    return "".join(alphabet[int(x)] for x in rng.integers(0, len(alphabet), n))


def make_case(rng, left, mature, right, r0, r1, iv, subs=(), n_at=(), lib_flank=("AC", "ACGTAC")):
    """A read lying at [r0, r1) of the precursor left + mature + right: the precursor's own bases (random ones outside
    it), then substitutions at read indices `subs` and N at `n_at`."""
    P = left + mature + right
    m0 = len(left)
    read = [P[x] if 0 <= x < len(P) and P[x] in "ACGT" else "ACGT"[int(rng.integers(0, 4))] for x in range(r0, r1)]
    for i in subs:
        if 0 <= i < len(read):
            read[i] = "ACGT"[("ACGT".index(read[i]) + 1 + int(rng.integers(0, 3))) % 4]
    for i in n_at:
        if 0 <= i < len(read):
            read[i] = "N"
    e0 = m0 - 2
    start = r0 - e0 + (1 if iv == 0 else 2)
    return (P, lib_flank[0] + mature + lib_flank[1], "".join(read), start, iv)


def enumerated_cases():
    rng = np.random.default_rng(20260)
    cases = []
    M = "TGAGGTAGTAGGTTGTATAGTT"
    # reads hanging off either end of the precursor (r0 < 0, r1 > len P, both), e0 < 0, all shifts around mature
    for left in (0, 1, 2, 5):
        for right in (0, 3, 10):
            L, Rt = rnd_seq(rng, left), rnd_seq(rng, right)
            for iv in (0, 8):
                for r0 in range(left - 3, left + 2):
                    for r1 in range(left + len(M) - 2, left + len(M) + 9):
                        cases.append(make_case(rng, L, M, Rt, r0, r1, iv))
    # the first mismatch at every position of the overlap: every reachable x - frame0, frame0 zero and negative, and
    # frame0 = r0 for the isomiR pass
    reached = set()
    for left in (0, 1, 2, 3, 7):
        L, Rt = rnd_seq(rng, left), rnd_seq(rng, 12)
        for iv in (0, 8):
            for r0 in (left - 3, left - 2, left, left + 1):
                for j in range(len(M)):
                    if left + j < r0:
                        continue
                    cases.append(make_case(rng, L, M, Rt, r0, left + len(M), iv, subs=(left + j - r0,)))
                    frame0 = min(0, left - 2) if iv == 0 else min(0, left - 2, r0)
                    reached.add(left + j - frame0)
                    # ... with a second one behind it (the FIRST decides)
                    cases.append(make_case(rng, L, M, Rt, r0, left + len(M), iv, subs=(left + j - r0, len(M) - 1 + left - r0)))
    assert {6, 7, 8, 11, 12, 16, 17} <= reached and min(reached) == 2
    L, Rt = rnd_seq(rng, 9), rnd_seq(rng, 15)
    for iv in (0, 8):
        m0, m1 = 9, 9 + len(M)
        cases += [
            make_case(rng, L, M, Rt, m0 - 2, m1, iv),                          # a 5' extension that matches
            make_case(rng, L, M, Rt, m0 - 2, m1, iv, subs=(5,)),               # ... behind an overlap mismatch
            make_case(rng, L, M, Rt, m0 - 2, m1, iv, subs=(0,)),               # one that differs
            make_case(rng, L, M, Rt, m0 - 2, m1, iv, subs=(1, 5)),             # ... after an overlap mismatch: class reset
            make_case(rng, L, M, Rt, m0, m1 + 3, iv),                          # a 3' extension that matches: iso_3p
            make_case(rng, L, M, Rt, m0, m1 + 3, iv, subs=(len(M) + 1,)),      # one that differs: iso_add
            make_case(rng, L, M, Rt, m0 + 2, m1 - 3, iv),                      # shorter than mature on both sides
            make_case(rng, L, M, Rt, m0 + 2, m1 - 3, iv, subs=(4,)),
            make_case(rng, L, M, Rt, m0, m1, iv),                              # the reference sequence itself
            make_case(rng, L, M, Rt, m0, m1, iv, n_at=(0,)),                   # read N at the first,
            make_case(rng, L, M, Rt, m0, m1, iv, n_at=(len(M) - 1,)),          # the last
            make_case(rng, L, M, Rt, m0, m1, iv, n_at=(10,)),                  # and a middle base
            make_case(rng, L, M, Rt, m0 - 1, m1 + 2, iv, n_at=(0, len(M) + 2)),
        ]
        # precursor N under a read N (equal) and under a base (differs): in the 3' extension and inside mature
        RtN = Rt[:1] + "N" + Rt[2:]
        MN = M[:8] + "N" + M[9:]
        cases += [
            make_case(rng, L, M, RtN, m0, m1 + 3, iv, n_at=(len(M) + 1,)),
            make_case(rng, L, M, RtN, m0, m1 + 3, iv),
            make_case(rng, L, MN, Rt, m0, m1, iv, n_at=(8,)),
            make_case(rng, L, MN, Rt, m0, m1, iv),
            make_case(rng, L, MN, Rt, m0 - 1, m1 + 1, iv, n_at=(9,), subs=(3,)),
        ]
    # read lengths across the word boundaries, against a long precursor
    L, Rt = rnd_seq(rng, 40), rnd_seq(rng, 300)
    for n in (16, 31, 32, 33, 63, 64, 65, 128, 255):
        for iv in (0, 8):
            for r0 in (40, 38, 41):
                cases.append(make_case(rng, L, M, Rt, r0, r0 + n, iv))
                cases.append(make_case(rng, L, M, Rt, r0, r0 + n, iv, subs=(n - 1,)))
                cases.append(make_case(rng, L, M, Rt, r0, r0 + n, iv, subs=(31, 32, 63, 64, 127, 128, 200), n_at=(n - 2,)))
    # ... and hanging off a short one at both ends
    for n in (33, 64, 65, 128, 255):
        cases.append(make_case(rng, "ACG", M, "TTGCA", -2, n - 2, 8))
        cases.append(make_case(rng, "ACG", M, "TTGCA", 1, n + 1, 0, subs=(7,)))
    return cases


def random_cases(n, seed):
    """Substitutions, shifts of -4 .. +4 at both ends, N at 2 % of the bases."""
    rng = np.random.default_rng(seed)
    cases = []
    for _ in range(n):
        left, right = int(rng.integers(0, 13)), int(rng.integers(0, 13))
        M = rnd_seq(rng, int(rng.integers(18, 26)))
        r0, r1 = left + int(rng.integers(-4, 5)), left + len(M) + int(rng.integers(-4, 5))
        L = r1 - r0
        subs = tuple(int(x) for x in rng.integers(0, L, int(rng.integers(0, 4))))
        n_at = tuple(int(x) for x in np.nonzero(rng.random(L) < 0.02)[0])
        cases.append(make_case(rng, rnd_seq(rng, left), M, rnd_seq(rng, right), r0, r1, 0 if rng.random() < 0.5 else 8,
                               subs=subs, n_at=n_at))
    return cases


@pytest.fixture(scope="module")
def edge_cases():
    return enumerated_cases()


@pytest.mark.parametrize("W", [1, 2, 4, 8])
def test_enumerated_edges_against_classify_alignment(gpu, edge_cases, W):
    cases = [c for c in edge_cases if len(c[2]) <= 32 * W]
    assert {len(c[2]) for c in cases} >= {n for n in (16, 31, 32, 33, 63, 64, 65, 128, 255) if n <= 32 * W}
    got = run_cases(gpu, cases, W, decode_all=True)
    if W == 1:   # what the enumeration is for: every class and every variant kind came out
        kinds = set()
        for g in got:
            kinds.update(v.split(":")[0] for v in g[1].split(","))
        assert {"NA", "iso_snp", "iso_snp_seed", "iso_snp_central_offset", "iso_snp_central", "iso_snpcentral_supp", "iso_add",
                "iso_5p", "iso_3p"} <= kinds
        assert any(g[2] <= 0 for g in got) and any("I" in g[4] for g in got)


def test_20000_random_cases(gpu):
    cases = random_cases(20000, 77)
    assert max(len(c[2]) for c in cases) == 33 and sum("N" in c[2] for c in cases) > 5000
    run_cases(gpu, cases, 2)
    run_cases(gpu, [c for c in cases if len(c[2]) <= 32][:5000], 1)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4095, 4096, 4097, 70001])
def test_selection_and_order(gpu, n):
    mature = "TGAGGTAGTAGGTTGTATAGTT"
    table = isomir.entry_table(["m"], ["AC" + mature + "TTAGGG"], {"m_pre": "GGGATGAGAC" + mature + "TTAGGGTCACACCCACC"}, {},
                               "MirGeneDB")
    rng = np.random.default_rng(n)
    words, lens, nmask = pack.pack_reads([mature], 1)
    words, lens = np.repeat(words, n, axis=1), np.repeat(lens, n)
    ref_id, pos = np.zeros(n, dtype=np.int32), np.full(n, 2, dtype=np.int32)
    others = np.array([-1, 1, 2, 3, 4, 5, 6, 7, 9], dtype=np.int8)
    for label in ("none", "sparse", "all"):
        if label == "none":
            pass_id = others[rng.integers(0, len(others), n)]
        elif label == "all":
            pass_id = np.where(rng.random(n) < 0.5, 0, 8).astype(np.int8)
        else:
            pass_id = others[rng.integers(0, len(others), n)]
            hit = rng.random(n) < 0.001
            hit[n // 2] = True
            pass_id[hit] = np.where(rng.random(int(hit.sum())) < 0.5, 0, 8)
        want = np.concatenate([np.nonzero(pass_id == 0)[0], np.nonzero(pass_id == 8)[0]]).astype(np.uint32)
        n_canon = int((pass_id == 0).sum())
        k = len(want)
        for pad in (0, 5):
            idx, rec, mask, a, b = gpu.classify(table, words, lens, None, pass_id, ref_id, pos, pad=pad)
            assert (a, b) == (n_canon, k - n_canon), label
            assert np.array_equal(idx, want), label
            kind = rec[:, 4] & 255
            # (pos 2 in the exact pass is the mature itself; the isomiR pass reads the same offset one base earlier)
            assert (kind[:n_canon] == isomir.KIND_REF).all() and (kind[n_canon:] == isomir.KIND_ISOMIR).all()
            assert not mask[:n_canon].any() and (rec[:, 6] == 0).all()
        if k:   # a capacity one short: the counts say so, the rows below it are the same, nothing behind it is written
            idx, rec, mask, a, b = gpu.classify(table, words, lens, None, pass_id, ref_id, pos, cap=k - 1)
            assert a + b == k and len(idx) == k - 1 and np.array_equal(idx, want[:k - 1])
            assert ((rec[:, 4] & 255) != 0).all()
    # other pass numbers: the two passes are arguments
    pass_id = rng.integers(-1, 10, n).astype(np.int8)
    idx, rec, mask, a, b = gpu.classify(table, words, lens, None, pass_id, ref_id, pos, canon=3, iso=5)
    assert np.array_equal(idx, np.concatenate([np.nonzero(pass_id == 3)[0], np.nonzero(pass_id == 5)[0]]))


def test_entries_that_cannot_be_resolved_and_bad_arguments(gpu):
    mature = "TGAGGTAGTAGGTTGTATAGTT"
    names = ["ok", "nohairpin", "notfound"]
    table = isomir.entry_table(names, ["AC" + mature + "TTAGGG"] * 3,
                               {"ok_pre": "GGGATGAGAC" + mature + "TTAGGG", "notfound_pre": "ACGT" * 12}, {}, "MirGeneDB")
    words, lens, nmask = pack.pack_reads([mature] * 6, 1)
    pass_id = np.array([0, 0, 0, 8, 0, 0], dtype=np.int8)
    ref_id = np.array([0, 1, 2, 0, 3, -1], dtype=np.int32)       # (3 and -1: no such entry)
    idx, rec, mask, a, b = gpu.classify(table, words, lens, nmask, pass_id, ref_id, np.full(6, 2))
    assert idx.tolist() == [0, 1, 2, 4, 5, 3]
    assert (rec[:, 4] & 255).tolist() == [isomir.KIND_REF, isomir.KIND_UNRESOLVABLE, isomir.KIND_DROPPED, isomir.KIND_BAD,
                                          isomir.KIND_BAD, isomir.KIND_ISOMIR]
    with pytest.raises(KeyError):
        isomir.raise_unresolved(table, rec)
    isomir.raise_unresolved(table, rec[[0, 2, 5]])
    # the wrapper takes host arrays as well as tensors
    got = gpu.eng.isomir_classify(table, words, lens, nmask, pass_id, ref_id, np.full(6, 2, dtype=np.int32))
    assert np.array_equal(got[0], idx) and np.array_equal(got[1], rec) and np.array_equal(got[2], mask) and got[3:] == (5, 1)
    # arguments
    L, h = gpu.lib, gpu.eng._h
    counts = (C.c_uint64 * 2)()
    d = gpu.up(np.zeros(64, dtype=np.int64))
    p = d.data_ptr()
    desc = np.ascontiguousarray(table.desc)
    args = lambda W=1, canon=0, iso=8, desc_ptr=desc.ctypes.data: (   # noqa: E731
        h, p, W, 6, p, None, 6, p, p, p, canon, iso, desc_ptr, 3, table.words.ctypes.data, table.nplane.ctypes.data,
        table.words.shape[0], 0, None, None, None, counts, None, None)
    assert L.mrg_isomir_classify(*args()) == 0
    for W in (0, 3, 5, 6, 7, 9, 16):
        assert L.mrg_isomir_classify(*args(W=W)) < 0 and b"words_per_read" in L.mrg_last_error()
    assert L.mrg_isomir_classify(*args(canon=8)) < 0
    assert L.mrg_isomir_classify(*args(desc_ptr=None)) < 0 and b"null" in L.mrg_last_error()
    broken = desc.copy()
    broken[0, 1] = 10 ** 6          # a precursor that ends outside the text
    assert L.mrg_isomir_classify(*args(desc_ptr=broken.ctypes.data)) < 0 and b"outside" in L.mrg_last_error()
    a6 = list(args())
    a6[17] = 6                      # a capacity without output buffers
    assert L.mrg_isomir_classify(*a6) < 0 and b"null output" in L.mrg_last_error()


def test_golden_world_through_the_engine_and_the_writer(gpu, golden, tmp_path):
    from mirge_amd import columnar
    from tests.test_isomir_native import golden_rows, golden_table, python_route
    names, seqs, hairpin, table = golden_table(golden)
    rows = golden_rows(golden)
    ref_dir = tmp_path / "py"
    ref_dir.mkdir()
    content, seq_dic = python_route(golden, rows, ref_dir)
    # the arrays: the two passes riffled together, each keeping its order; some reads of other passes in between
    rng = np.random.default_rng(5)
    canon, iso = [r for r in rows if r[3] == 0], [r for r in rows if r[3] == 8]
    order, a, b = [], 0, 0
    while a < len(canon) or b < len(iso):
        pick = rng.integers(0, 3)
        if pick == 0 and a < len(canon):
            order.append(canon[a])
            a += 1
        elif pick == 1 and b < len(iso):
            order.append(iso[b])
            b += 1
        else:
            order.append(("ACGTTGCAACGTTGCAACGT" + rnd_seq(rng, 8), None, 1, 4))
    seqs_in = [r[0] for r in order]
    words, lens, nmask = pack.pack_reads(seqs_in)
    assert nmask is not None
    pass_id = np.array([r[3] for r in order], dtype=np.int8)
    ref_id = np.array([names.index(r[1]) if r[1] else 0 for r in order], dtype=np.int32)
    pos = np.array([r[2] - 1 for r in order], dtype=np.int32)
    quant = np.array([seq_dic[s]["quant"] if s in seq_dic else [3, 3] for s in seqs_in], dtype=np.uint32)
    timings = {}
    idx, rec, mask, n_canon, n_iso = gpu.eng.isomir_classify(table, words, lens, nmask, pass_id, ref_id, pos, timings=timings)
    assert (n_canon, n_iso) == (len(canon), len(iso)) and 0 < timings["kernel_ms"] <= timings["classify_call_ms"]
    assert [seqs_in[i] for i in idx.tolist()] == [r[0] for r in rows]
    out = tmp_path / "native"
    out.mkdir()
    lines = columnar.write_isomir_gff(str(out), golden["sample_list"], words, lens, nmask, quant, idx, rec, mask, table, names,
                                      "miRBase")
    for fn, want in golden["expected"]["gff_files"].items():
        got = open(str(out / fn)).read()
        assert got == open(str(ref_dir / fn)).read(), fn
        got = got.split("\n")
        assert got[:4] == want[:4] and sorted(got[4:]) == sorted(want[4:])
    assert sum(lines) == sum(len(v) - 5 for v in golden["expected"]["gff_files"].values())


def write_world(tmp_path, long_entry=False):
    """A SynthLibraries world with SNP and SNPC entries in the miRge.Libs layout, its miRBase-style gff3, and two samples
    whose reads include N and the SNP entries' own matures."""
    from mirge_amd import synth
    from tests.golden.make_golden import SHAPES
    from tests.test_cli import write_fastq
    rng = np.random.default_rng(31)
    libs = synth.SynthLibraries(seed=123, scale=1.0, n_paralogs=6, n_snp=8, shapes=SHAPES, snpc=True)
    names, seqs = libs.libs["mirna"]
    long_read = None
    if long_entry:   # a miRNA entry long enough for a read beyond 255 nt, which only the isomiR pass can claim
        body = rnd_seq(rng, 300)
        names.append("syn-miR-9999-5p")
        seqs.append(body)
        libs.libs["hairpin"][0].append("syn-mir-9999")
        libs.libs["hairpin"][1].append(rnd_seq(rng, 20) + body + rnd_seq(rng, 20))
        flip = {"A": "C", "C": "G", "G": "T", "T": "A"}
        long_read = flip[body[9]] + body[10:270] + flip[body[270]] + flip[body[271]]
    root = str(tmp_path / "libs")
    libs.write_layout(root, species="syn", db="miRBase")
    with open(os.path.join(root, "syn", "annotation.Libs", "syn_miRBase.gff3"), "w") as fh:
        fh.write("##gff-version 3\n")
        for h, hp in enumerate(libs.libs["hairpin"][0]):
            fh.write("chr1\t.\tmiRNA_primary_transcript\t1\t90\t.\t+\t.\tID=MI%d;Alias=MI%d;Name=%s\n" % (h, h, hp))
        seen = set()
        for name in names:
            canonical = name.split(".")[0]
            if canonical in seen:
                continue
            seen.add(canonical)
            h = libs.libs["hairpin"][0].index("syn-mir-" + canonical.split("-")[2])
            fh.write("chr1\t.\tmiRNA\t1\t22\t.\t+\t.\tID=MIMAT%d;Alias=MIMAT%d;Name=%s;Derives_from=MI%d\n"
                     % (len(seen), len(seen), canonical, h))
    snp_matures = [s[2:-6] for n, s in zip(names, seqs) if ".SNP" in n]
    assert len(snp_matures) >= 8
    fastqs = []
    for si in range(2):
        reads = [synth.codes_to_str(c) for c in synth.synth_reads(libs, 1500, seed=40 + si, zipf_s=1.3)]
        reads += snp_matures + [m[:5] + "N" + m[6:] for m in snp_matures[si::2]] + [m[1:] + "A" for m in snp_matures]
        reads += ["ACGTNACGTTAGCATCGATCGA", "TTTTTTTTTTTTTTTTTTTT"]
        if long_read:
            reads += [long_read] * (si + 1)
        p = str(tmp_path / ("s%d.fastq" % si))
        write_fastq(p, reads, rng)
        fastqs.append(p)
    return root, fastqs, long_read


def run_gff(tmp_path, root, fastqs, label, extra=()):
    from mirge_amd import cli
    out = tmp_path / label
    out.mkdir()
    res = cli.annotate_main(cli.build_parser().parse_args(
        ["annotate", "-s"] + fastqs + ["-lib", root, "-sp", "syn", "-o", str(out), "-gff", "-ad", "none"] + list(extra)))
    files = {fn: open(os.path.join(res["outdir"], fn), "rb").read() for fn in sorted(os.listdir(res["outdir"]))
             if fn.endswith("_isomiRs.gff")}
    assert sorted(files) == ["s0_isomiRs.gff", "s1_isomiRs.gff"]
    return files


def test_annotate_gff_writes_the_same_files_on_both_routes(native_lib, tmp_path, monkeypatch):
    from mirge_amd import columnar
    root, fastqs, _ = write_world(tmp_path)
    calls = []
    real = columnar.write_isomir_gff
    monkeypatch.setattr(columnar, "write_isomir_gff", lambda *a, **k: calls.append(1) or real(*a, **k))
    new = run_gff(tmp_path, root, fastqs, "new")
    assert calls == [1]
    old = run_gff(tmp_path, root, fastqs, "old", ["--gff-host"])
    assert calls == [1]
    assert new == old
    body = new["s0_isomiRs.gff"].decode().split("\n")
    assert len(body) > 200 and body[3] == "## COLDATA: s0"
    text = new["s0_isomiRs.gff"].decode() + new["s1_isomiRs.gff"].decode()
    assert ".SNP" in text and "\tref_miRNA\t" in text and "iso_snp" in text and " UID .;" in text and "iso_add" in text


def test_annotate_gff_with_a_long_mirna_read_takes_the_record_route(native_lib, tmp_path, monkeypatch):
    from mirge_amd import columnar
    root, fastqs, long_read = write_world(tmp_path, long_entry=True)
    assert len(long_read) == 263
    calls = []
    monkeypatch.setattr(columnar, "write_isomir_gff", lambda *a, **k: calls.append(1))
    new = run_gff(tmp_path, root, fastqs, "new")
    old = run_gff(tmp_path, root, fastqs, "old", ["--gff-host"])
    assert calls == [] and new == old
    line = [ln for ln in new["s1_isomiRs.gff"].decode().split("\n") if "Read " + long_read + ";" in ln]
    assert len(line) == 1 and line[0].startswith("syn-miR-9999-5p\tmiRBase22\tisomiR\t") and line[0].endswith("Expression 2; Filter Pass")
