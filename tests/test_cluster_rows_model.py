"""CPU: the array-level cluster model (tests/cluster_rows_model.py) against the text model the suite already trusts
(tests/predict_cluster_model.py) on random row sets, both against clusters written out by hand, and the argument checks
of the mrg_cluster_* entry points that fail before any device call."""
import ctypes as C

import numpy as np
import pytest

from tests import cluster_rows_model as model
from tests import predict_cluster_model as text_model


def sam_text(kw):
    """The rows as a coordinate-sorted SAM file: kept entries are chr<e>, masked ones scaffold_<e>, reads mir<r>_<count>."""
    keep = kw["entry_keep"]
    rows = model.ordered(model.flat_rows(kw["parts"], kw["n_entries"], None), model.SAM_ORDER)
    lines = []
    for _, e, pos, strand, r, _ in rows:
        seq = model.revcomp(kw["reads"][r]) if strand else kw["reads"][r]
        chrom = ("chr%d" if keep is None or keep[e] else "scaffold_%d") % e
        lines.append("\t".join(["mir%d_%d" % (r, int(kw["counts"][r])), "16" if strand else "0", chrom, str(pos + 1), "255",
                                "%dM" % len(seq), "*", "0", "0", seq, "I" * len(seq)]))
    return "\n".join(lines) + "\n"


def tsv_fields(m, kw):
    """The array model's clusters as the lines of the cluster table, without the header."""
    out = []
    for c in range(m["n_clusters"]):
        a, b = int(m["member_off"][c]), int(m["member_off"][c + 1])
        seq = m["seq"][int(m["seq_off"][c]):int(m["seq_off"][c + 1])].decode()
        out.append(["s:miRCluster_%d_%d" % (c + 1, len(seq)), "chr%d" % m["entry"][c], "+-"[m["strand"][c]], str(m["start"][c]),
                    str(m["end"][c]), seq, str(int(m["len"][c])), str(m["sum"][c]), str(b - a),
                    ",".join("mir%d_%d" % (r, int(kw["counts"][r])) for r in m["member"][a:b])])
    return out


@pytest.mark.parametrize("block", range(8))
def test_array_model_equals_the_text_model(block):
    """240 random row sets (30 a block): every field of every line of the text model's table, the member lists
    included, from the arrays; lengths to 255, thresholds 1..40, counts to 2^32 - 1."""
    for seed in range(30 * block, 30 * block + 30):
        rng = np.random.default_rng(seed)
        t = int(rng.choice([1, 2, 5, 14, 15, 40]))
        kw = model.random_rows(rng, int(rng.integers(1, 400)), t, max_len=int(rng.choice([20, 32, 64, 128, 255])),
                               n_entries=int(rng.integers(2, 7)), n_parts=int(rng.integers(1, 3)), masked=int(rng.integers(0, 2)),
                               max_count=int(rng.choice([97, 2 ** 32 - 1])))
        m = model.cluster_rows(**kw)
        want = [l.split("\t") for l in text_model.cluster_tsv(sam_text(kw), t, "s").splitlines()[1:]]
        assert tsv_fields(m, kw) == want, seed
        assert len(m["seq"]) == int(m["seq_off"][-1]) == int(m["len"].sum()) and m["len"][-1] == 0
        assert np.array_equal(m["len"][:-1], m["end"] - m["start"] + 1)


def test_random_rows_draws_every_kind():
    """The generator's mix: over a few sets there are duplicates, shared positions, contained and abutting rows, the
    three overlaps around the threshold, reads below the threshold, multi-row clusters and single-row ones."""
    seen = set()
    for seed in range(20):
        t = 14
        kw = model.random_rows(np.random.default_rng(seed), 300, t, max_len=64)
        m = model.cluster_rows(**kw)
        read, entry, pos, strand, _ = (x.tolist() for x in m["rows_cluster"])
        L = [len(kw["reads"][r]) for r in read]
        E = None
        for i in range(m["n_valid"]):
            s, e = pos[i] + 1, pos[i] + L[i]
            if i and (entry[i], strand[i]) == (entry[i - 1], strand[i - 1]) and E is not None:
                if (read[i], pos[i]) == (read[i - 1], pos[i - 1]):
                    seen.add("duplicate")
                elif pos[i] == pos[i - 1]:
                    seen.add("same position")
                if e <= E and s <= E:
                    seen.add("contained")
                if s == E + 1:
                    seen.add("abutting")
                if E - s + 1 in (t - 1, t, t + 1):
                    seen.add("overlap %+d" % (E - s + 1 - t))
                if L[i] < t:
                    seen.add("short")
                E = max(E, e)
            else:
                E = e
        n_members = np.diff(m["member_off"].astype(np.int64))
        if (n_members > 3).any() and (n_members == 1).any():
            seen.add("sizes")
    assert seen == {"duplicate", "same position", "contained", "abutting", "overlap -1", "overlap +0", "overlap +1", "short", "sizes"}


# ------------------------------------------------------------------------------------------------ by hand
R0 = "AAAAACCCCCGGGGGTTTTT"      # its own reverse complement
R1 = "CATCATCATCATCATCATGA"      # reverse complement TCATGATGATGATGATGATG
R2 = "GG"
R3 = "ACN"                       # reverse complement NGT
HAND_READS = [R0, R1, R2, R3]
HAND_COUNTS = [3, 5, 7, 4000000000]

# (rows (read, offset, strand), threshold) -> clusters (strand, start, end, sequence, members, sum)
HAND = {
    "overlap t joins": ([(0, 0, 0), (1, 6, 0)], 14, [(0, 1, 26, R0 + "TCATGA", [0, 1], 8)]),
    "overlap t - 1 does not": ([(0, 0, 0), (1, 6, 0)], 15, [(0, 1, 20, R0, [0], 3), (0, 7, 26, R1, [1], 5)]),
    "overlap t + 1 joins": ([(0, 0, 0), (1, 6, 0)], 13, [(0, 1, 26, R0 + "TCATGA", [0, 1], 8)]),
    "s = E joins at 1": ([(0, 0, 0), (1, 19, 0)], 1, [(0, 1, 39, R0 + R1[1:], [0, 1], 8)]),
    "s = E not at 2": ([(0, 0, 0), (1, 19, 0)], 2, [(0, 1, 20, R0, [0], 3), (0, 20, 39, R1, [1], 5)]),
    "s = E + 1 never": ([(0, 0, 0), (1, 20, 0)], 1, [(0, 1, 20, R0, [0], 3), (0, 21, 40, R1, [1], 5)]),
    "e = E and e < E add a member, no base": ([(0, 0, 0), (2, 18, 0), (2, 3, 0)], 1, [(0, 1, 20, R0, [0, 2, 2], 17)]),
    "identical rows": ([(1, 4, 0), (1, 4, 0)], 14, [(0, 5, 24, R1, [1, 1], 10)]),
    # at offset 10 read 1 comes before read 2 whatever the row order: it opens [11, 30] (10 < 14 bases of [1, 20]) and read 2 joins IT
    "ties are in read order": ([(2, 10, 0), (0, 0, 0), (2, 3, 0), (1, 10, 0)], 14,
                               [(0, 1, 20, R0, [0, 2], 10), (0, 11, 30, R1, [1, 2], 12)]),
    # GG at [10, 11] has 11 bases of [1, 20]: a cluster of its own that ends before 20; R1 at [13, 32] starts behind it
    "a short cluster ends before the long one": ([(0, 0, 0), (2, 9, 0), (1, 12, 0)], 14,
                                                 [(0, 1, 20, R0, [0], 3), (0, 10, 11, R2, [2], 7), (0, 13, 32, R1, [1], 5)]),
    # ... and without the short one in between R1 has 8 bases of [1, 20] and still does not join
    "the same without it": ([(0, 0, 0), (1, 12, 0)], 14, [(0, 1, 20, R0, [0], 3), (0, 13, 32, R1, [1], 5)]),
    # GG inside [1, 20] with 17 bases to its end joins although it is shorter than the threshold
    "a short read inside joins": ([(0, 0, 0), (2, 3, 0), (1, 6, 0)], 14, [(0, 1, 26, R0 + "TCATGA", [0, 2, 1], 15)]),
    "minus strand": ([(1, 0, 1), (0, 6, 1)], 14, [(1, 1, 26, "TCATGATGATGATGATGATG" + "GTTTTT", [1, 0], 8)]),
    "strands are lists of their own": ([(0, 0, 0), (1, 6, 1), (3, 2, 1)], 1,
                                       [(0, 1, 20, R0, [0], 3), (1, 3, 5, "NGT", [3], 4000000000),
                                        (1, 7, 26, "TCATGATGATGATGATGATG", [1], 5)]),
    "N is kept": ([(3, 0, 0), (3, 1, 1)], 1, [(0, 1, 3, "ACN", [3], 4000000000), (1, 2, 4, "NGT", [3], 4000000000)]),
    "the sum passes 2^32": ([(3, 0, 0), (3, 0, 0), (3, 1, 0)], 1, [(0, 1, 4, "ACNN", [3, 3, 3], 12000000000)]),
}


def hand_input(rows, t):
    rows = [(r, 0, pos, strand, 0) for r, pos, strand in rows]
    return dict(parts=model.make_parts(rows, len(HAND_READS), [0], 1), reads=HAND_READS, counts=HAND_COUNTS, entry_keep=None,
                n_entries=1, threshold=t)


@pytest.mark.parametrize("name", sorted(HAND))
def test_clusters_written_out_by_hand(name):
    rows, t, want = HAND[name]
    kw = hand_input(rows, t)
    m = model.cluster_rows(**kw)
    got = [(int(m["strand"][c]), int(m["start"][c]), int(m["end"][c]),
            m["seq"][int(m["seq_off"][c]):int(m["seq_off"][c + 1])].decode(),
            m["member"][int(m["member_off"][c]):int(m["member_off"][c + 1])].tolist(), m["sum"][c]) for c in range(m["n_clusters"])]
    assert got == want
    lines = [l.split("\t") for l in text_model.cluster_tsv(sam_text(kw), t, "s").splitlines()[1:]]
    assert [("+-".index(f[2]), int(f[3]), int(f[4]), f[5], [int(x[3:].split("_")[0]) for x in f[9].split(",")], int(f[7]))
            for f in lines] == want


def test_masked_rows_sort_last_and_keep_their_entry_in_sam_order():
    """Two entries, the first masked: by hand."""
    rows = [(0, 0, 5, 0, 1), (1, 1, 9, 1, 2), (1, 1, 9, 0, 0), (2, 0, 1, 1, 0)]
    kw = dict(parts=model.make_parts(rows, 4, [0, 1], 2), reads=HAND_READS, counts=HAND_COUNTS,
              entry_keep=np.array([0, 1], np.uint8), n_entries=2, threshold=14)
    m = model.cluster_rows(**kw)
    assert [x.tolist() for x in m["rows_cluster"]] == [[1, 1, 0, 2], [1, 1, 2, 2], [9, 9, 5, 1], [0, 1, 0, 1], [0, 2, 1, 0]]
    assert [x.tolist() for x in m["rows_sam"]] == [[2, 0, 1, 1], [0, 0, 1, 1], [1, 5, 9, 9], [1, 0, 0, 1], [0, 1, 0, 2]]
    assert (m["n_rows"], m["n_valid"], m["n_clusters"]) == (4, 2, 2) and m["member"].tolist() == [1, 1]
    assert m["member_off"].tolist() == [0, 1, 2] and m["entry"].tolist() == [1, 1] and m["strand"].tolist() == [0, 1]


# ------------------------------------------------------------------------------------------------ argument checks
def test_cluster_entry_points_refuse_bad_arguments(native_lib):
    """Every refusal below comes before the first device call: no GPU is needed, and the pointers are never followed."""
    L = native_lib
    x = C.c_void_p(8)
    big = 2 ** 32 - 1
    tmp_b, work_b = C.c_uint64(), C.c_uint64()
    assert L.mrg_cluster_workspace_bytes(10, C.byref(tmp_b), C.byref(work_b)) == 0 and tmp_b.value > 0 and work_b.value > 0
    assert L.mrg_cluster_workspace_bytes(10, None, C.byref(work_b)) < 0 and b"null" in L.mrg_last_error()
    tb, wb = tmp_b.value, work_b.value
    second, nv, nc, total = C.c_int32(), C.c_uint64(), C.c_uint64(), C.c_uint64()

    def keys(ctx=x, rows=10, row_base=0, total_rows=10, n_entries=5, pos_bits=20, order=0):
        return L.mrg_cluster_keys(ctx, x, 3, x, x, x, rows, row_base, total_rows, 0, n_entries, pos_bits, order, None, x, x, x, None)

    def sort(ctx=x, rows=10, bits=30, tmp_bytes=tb):
        return L.mrg_cluster_sort(ctx, x, x, x, x, rows, bits, x, tmp_bytes, C.byref(second), None)

    def scan(ctx=x, rows=10, n_entries=5, pos_bits=20, t=14, work_bytes=wb, tmp_bytes=tb):
        return L.mrg_cluster_scan(ctx, x, x, rows, x, x, n_entries, pos_bits, t, x, work_bytes, x, tmp_bytes, x, C.byref(nv),
                                  C.byref(nc), None)

    def bounds(ctx=x, rows=10, n_valid=8, n_clusters=4, pos_bits=20, work_bytes=wb, tmp_bytes=tb):
        return L.mrg_cluster_bounds(ctx, x, rows, n_valid, n_clusters, pos_bits, x, work_bytes, x, tmp_bytes, x, x, x, x, x, x, x,
                                    C.byref(total), None)

    def assemble(ctx=x, rows=10, n_valid=8, n_clusters=4, pos_bits=20, work_bytes=wb):
        return L.mrg_cluster_assemble(ctx, x, rows, n_valid, n_clusters, pos_bits, x, work_bytes, x, x, 1, x, None, 3, x, x, x, x, x,
                                      None)

    def gather(ctx=x, rows=10, pos_bits=20, order=1):
        return L.mrg_cluster_sorted_rows(ctx, x, x, rows, pos_bits, order, x, x, x, x, x, x, x, None)

    def refused(rc, word):
        assert rc < 0
        assert word in L.mrg_last_error(), L.mrg_last_error()

    for f in (keys, sort, scan, bounds, assemble, gather):
        refused(f(ctx=None), b"null")
    refused(keys(rows=0, total_rows=big), b"2^32 - 2")
    for f in (sort, scan, bounds, assemble, gather):
        refused(f(rows=big), b"2^32 - 2")
    for f in (keys, scan, bounds, assemble, gather):
        for pb in (0, 32):
            refused(f(pos_bits=pb), b"pos_bits %d" % pb)
    for f in (keys, scan):
        refused(f(n_entries=big, pos_bits=31), b"entry bits")
    refused(keys(order=2), b"order 2")
    refused(gather(order=-1), b"order -1")
    refused(keys(rows=6, row_base=5), b"out of range")
    refused(keys(rows=1, row_base=10), b"out of range")
    refused(scan(t=0), b"threshold")
    refused(scan(t=-3), b"threshold")
    for f in (bounds, assemble):
        refused(f(n_valid=11), b"more clusters than rows")
        refused(f(n_valid=3, n_clusters=4), b"more clusters than rows")
    refused(sort(tmp_bytes=tb - 1), b"smaller")
    refused(scan(tmp_bytes=tb - 1), b"smaller")
    refused(scan(work_bytes=wb - 1), b"smaller")
    refused(bounds(tmp_bytes=tb - 1), b"smaller")
    refused(bounds(work_bytes=wb - 1), b"smaller")
    refused(assemble(work_bytes=wb - 1), b"smaller")
    refused(sort(bits=65), b"65 key bits")
    assert nv.value == 0 and nc.value == 0 and total.value == 0
