"""GPU (-m gpu): predict mode's location-cluster stages called directly -- mrg_cluster_keys once per part, then _sort,
_scan, _bounds, _assemble and _sorted_rows in both orders -- on hand-made alignment rows, against the sequential array
model (tests/cluster_rows_model.py, pinned by tests/test_cluster_rows_model.py).  Integers and bytes: every comparison
is exact.

Every output buffer has exactly the size the header states plus a guard of pattern bytes behind it, d_tmp and d_work
exactly the sizes mrg_cluster_workspace_bytes reports plus a guard; all guards are checked after every stage.  d_work,
d_tmp and d_seq are handed over full of the pattern: a slot nobody writes (n_valid, a base of a sequence) shows."""
import ctypes as C

import numpy as np
import pytest

from tests import cluster_rows_model as model

pytestmark = pytest.mark.gpu

GUARD = 256           # bytes behind every buffer
PAT = 0xA5            # every guard byte, and no letter of a sequence
CLUSTER_ORDER, SAM_ORDER = 0, 1


class Stages:
    def __init__(self):
        import torch
        from mirge_amd.engine import Engine
        self.torch = torch
        self.eng = Engine(0)
        self.lib = self.eng._lib
        self.dev = self.eng.device

    # -- buffers: bytes on the device, GUARD pattern bytes behind the payload
    def up(self, arr, name):
        arr = np.ascontiguousarray(arr)
        buf = np.full(arr.nbytes + GUARD, PAT, np.uint8)
        buf[:arr.nbytes] = arr.reshape(-1).view(np.uint8)
        t = self.torch.from_numpy(buf).to(self.dev)
        self.bufs.append((name, t, arr.nbytes))
        return t

    def blank(self, count, dtype, name):
        nbytes = int(count) * np.dtype(dtype).itemsize
        t = self.torch.full((nbytes + GUARD,), PAT, dtype=self.torch.uint8, device=self.dev)
        self.bufs.append((name, t, nbytes))
        return t

    def down(self, t, count, dtype):
        return t[:int(count) * np.dtype(dtype).itemsize].cpu().numpy().view(dtype)

    def guards(self, stage):
        """Synchronise; every guard of every buffer made so far must hold the pattern."""
        self.torch.cuda.current_stream(self.dev).synchronize()
        tails = self.torch.cat([t[n:] for _, t, n in self.bufs])
        if not bool((tails == PAT).all()):
            bad = [name for name, t, n in self.bufs if not bool((t[n:] == PAT).all())]
            raise AssertionError("%s wrote behind the end of %s" % (stage, ", ".join(bad)))

    def ok(self, rc):
        assert rc == 0, self.lib.mrg_last_error()

    def run(self, parts, reads, counts, entry_keep, n_entries, threshold, W=None, pos_bits=None, nmask="present", garbage=False):
        """All stages on one input -> what they left, shaped like the model's result."""
        from mirge_amd import pack
        lib, h, st = self.lib, self.eng._h, self.eng._stream_ptr()
        self.bufs = []
        n = len(reads)
        T = int(sum(len(p["ref"]) for p in parts))
        assert T > 0
        words, lens, nm = pack.pack_reads(reads, W)
        W = words.shape[0]
        if garbage:         # random bits in every word behind the read's last base
            rng = np.random.default_rng(99)
            for w in range(W):
                used = np.clip(lens.astype(np.int64) - 32 * w, 0, 32)
                keep = np.array([(1 << (2 * int(u))) - 1 for u in used], dtype=np.uint64)
                words[w] = (words[w] & keep) | (rng.integers(0, 2 ** 64, n, dtype=np.uint64) & ~keep)
        if nmask == "null":
            assert nm is None, "a read with an N needs the mask"
        elif nm is None:
            nm = np.zeros((W, n), np.uint64)
        d_words, d_lens = self.up(words, "reads"), self.up(lens, "lens")
        d_nm = self.up(nm, "nmask") if nm is not None else None
        d_counts = self.up(np.asarray(counts, dtype=np.uint32), "counts")
        d_keep = self.up(np.asarray(entry_keep, dtype=np.uint8), "entry_keep") if entry_keep is not None else None
        d_mm = self.up(np.concatenate([p["mm"] for p in parts]).astype(np.uint8), "mm")
        d_parts = [tuple(self.up(np.asarray(p[k], dtype=dt), k) for k, dt in
                         (("offsets", np.uint64), ("ref", np.int32), ("pos", np.int32), ("strand", np.uint8))) for p in parts]
        if pos_bits is None:
            pos_bits = max(1, int(max(int(p["pos"].max()) for p in parts if len(p["pos"]))).bit_length())
        bits = pos_bits + 1 + max(1, int(n_entries).bit_length())
        tmp_b, work_b = C.c_uint64(), C.c_uint64()
        self.ok(lib.mrg_cluster_workspace_bytes(T, C.byref(tmp_b), C.byref(work_b)))
        tmp, work = self.blank(tmp_b.value, np.uint8, "d_tmp"), self.blank(work_b.value, np.uint8, "d_work")
        k = [self.blank(T, np.uint64, "d_keys0"), self.blank(T, np.uint64, "d_keys1")]
        v = [self.blank(T, np.uint32, "d_vals0"), self.blank(T, np.uint32, "d_vals1")]
        owner = self.blank(T, np.uint32, "d_owner")
        want_owner = np.concatenate([np.repeat(np.arange(n, dtype=np.uint32), np.diff(p["offsets"].astype(np.int64))) for p in parts])

        def sorted_pairs(order, keep):
            row_base = 0
            for p, (d_off, d_ref, d_pos, d_strand) in zip(parts, d_parts):
                rows = len(p["ref"])
                self.ok(lib.mrg_cluster_keys(h, d_off.data_ptr(), n, d_ref.data_ptr(), d_pos.data_ptr(), d_strand.data_ptr(), rows,
                                             row_base, T, int(p["entry_base"]), n_entries, pos_bits, order,
                                             keep.data_ptr() if keep is not None else None, k[0].data_ptr(), v[0].data_ptr(),
                                             owner.data_ptr(), st))
                row_base += rows
            self.guards("mrg_cluster_keys")
            assert np.array_equal(self.down(owner, T, np.uint32), want_owner), "d_owner"
            assert np.array_equal(self.down(v[0], T, np.uint32), np.arange(T, dtype=np.uint32)), "d_vals"
            second = C.c_int32(-1)
            self.ok(lib.mrg_cluster_sort(h, k[0].data_ptr(), k[1].data_ptr(), v[0].data_ptr(), v[1].data_ptr(), T, bits,
                                         tmp.data_ptr(), tmp_b.value, C.byref(second), st))
            self.guards("mrg_cluster_sort")
            assert second.value in (0, 1)
            return k[second.value], v[second.value]

        def columns(order, sk, sv):
            out = [self.blank(T, dt, "sorted rows " + nm_) for nm_, dt in (("read", np.uint32), ("entry", np.int32), ("pos", np.int32),
                                                                           ("strand", np.uint8), ("mm", np.uint8))]
            self.ok(lib.mrg_cluster_sorted_rows(h, sk.data_ptr(), sv.data_ptr(), T, pos_bits, order, owner.data_ptr(), d_mm.data_ptr(),
                                                *[t.data_ptr() for t in out], st))
            self.guards("mrg_cluster_sorted_rows")
            r, e, p, s, m = (self.down(t, T, dt) for t, dt in zip(out, (np.uint32, np.int32, np.int32, np.uint8, np.uint8)))
            return r, e.view(np.uint32), p.astype(np.int64), s, m

        sk, sv = sorted_pairs(CLUSTER_ORDER, d_keep)
        member = self.blank(T, np.uint32, "d_member")
        n_valid, n_clusters = C.c_uint64(PAT), C.c_uint64(PAT)
        self.ok(lib.mrg_cluster_scan(h, sk.data_ptr(), sv.data_ptr(), T, owner.data_ptr(), d_lens.data_ptr(), n_entries, pos_bits,
                                     int(threshold), work.data_ptr(), work_b.value, tmp.data_ptr(), tmp_b.value, member.data_ptr(),
                                     C.byref(n_valid), C.byref(n_clusters), st))
        self.guards("mrg_cluster_scan")
        V, K = int(n_valid.value), int(n_clusters.value)
        assert K <= V <= T, "n_clusters %d, n_valid %d of %d rows" % (K, V, T)
        c_entry, c_start, c_end = (self.blank(K, np.uint32, "d_" + x) for x in ("entry", "start", "end"))
        c_strand = self.blank(K, np.uint8, "d_strand")
        c_moff, c_len = self.blank(K + 1, np.uint32, "d_member_off"), self.blank(K + 1, np.uint32, "d_len")
        c_soff = self.blank(K + 1, np.uint64, "d_seq_off")
        total = C.c_uint64(PAT)
        self.ok(lib.mrg_cluster_bounds(h, sk.data_ptr(), T, V, K, pos_bits, work.data_ptr(), work_b.value, tmp.data_ptr(), tmp_b.value,
                                       c_entry.data_ptr(), c_strand.data_ptr(), c_start.data_ptr(), c_end.data_ptr(), c_moff.data_ptr(),
                                       c_len.data_ptr(), c_soff.data_ptr(), C.byref(total), st))
        self.guards("mrg_cluster_bounds")
        seq = self.blank(total.value, np.uint8, "d_seq")
        c_sum = self.blank(K, np.uint64, "d_sum")
        self.ok(lib.mrg_cluster_assemble(h, sk.data_ptr(), T, V, K, pos_bits, work.data_ptr(), work_b.value, member.data_ptr(),
                                         d_words.data_ptr(), W, d_lens.data_ptr(), d_nm.data_ptr() if d_nm is not None else None, n,
                                         d_counts.data_ptr(), c_start.data_ptr(), c_soff.data_ptr(), seq.data_ptr(), c_sum.data_ptr(),
                                         st))
        self.guards("mrg_cluster_assemble")
        got = dict(n_rows=T, n_valid=V, n_clusters=K, total_len=int(total.value), W=W,
                   member_all=self.down(member, T, np.uint32),
                   entry=self.down(c_entry, K, np.uint32), strand=self.down(c_strand, K, np.uint8),
                   start=self.down(c_start, K, np.uint32), end=self.down(c_end, K, np.uint32),
                   member_off=self.down(c_moff, K + 1, np.uint32), len=self.down(c_len, K + 1, np.uint32),
                   seq_off=self.down(c_soff, K + 1, np.uint64), seq=self.down(seq, total.value, np.uint8).tobytes(),
                   sum=[int(x) for x in self.down(c_sum, K, np.uint64)])
        got["rows_cluster"] = columns(CLUSTER_ORDER, sk, sv)
        sk, sv = sorted_pairs(SAM_ORDER, None)
        got["rows_sam"] = columns(SAM_ORDER, sk, sv)
        return got


@pytest.fixture(scope="module")
def stages(native_lib):
    return Stages()


def first_diff(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape:
        return "shapes %s and %s" % (a.shape, b.shape)
    i = int(np.flatnonzero(a != b)[0])
    return "first at %d: got %s, want %s" % (i, a[i], b[i])


def compare(got, want, tag=""):
    """Everything the C API yields against the model, exactly."""
    for order in ("rows_cluster", "rows_sam"):
        for name, g, w in zip(("read", "entry", "offset", "strand", "mm"), got[order], want[order]):
            assert np.array_equal(g, w), "%s %s %s: %s" % (tag, order, name, first_diff(g, w))
    for name in ("n_rows", "n_valid", "n_clusters"):
        assert got[name] == want[name], "%s %s: got %d, want %d" % (tag, name, got[name], want[name])
    V = want["n_valid"]
    assert np.array_equal(got["member_all"][:V], want["member"]), "%s member: %s" % (tag, first_diff(got["member_all"][:V], want["member"]))
    assert np.array_equal(got["member_all"][V:], want["rows_cluster"][0][V:]), tag + " member of the masked rows"
    for name in ("entry", "strand", "start", "end", "member_off", "len", "seq_off"):
        assert np.array_equal(got[name], want[name]), "%s %s: %s" % (tag, name, first_diff(got[name], want[name]))
    assert got["total_len"] == len(want["seq"]), tag
    if got["seq"] != want["seq"]:
        g, w = np.frombuffer(got["seq"], np.uint8), np.frombuffer(want["seq"], np.uint8)
        i = int(np.flatnonzero(g != w)[0])
        c = int(np.searchsorted(want["seq_off"], i, side="right")) - 1
        raise AssertionError("%s seq: byte %d (cluster %d, base %d) is %r, want %r" % (
            tag, i, c, i - int(want["seq_off"][c]), bytes(g[i:i + 1]), bytes(w[i:i + 1])))
    assert got["sum"] == want["sum"], "%s sum: %s" % (tag, first_diff(np.array(got["sum"], object), np.array(want["sum"], object)))


def check(stages, kw, tag="", **how):
    want = model.cluster_rows(**kw)
    got = stages.run(**kw, **how)
    compare(got, want, tag)
    return got, want


def one_list(rows, reads, t, counts=None):
    """rows (read, offset[, strand]) on entry 0."""
    rows = [(r[0], 0, r[1], r[2] if len(r) > 2 else 0, (i * 7) % 3) for i, r in enumerate(rows)]
    return dict(parts=model.make_parts(rows, len(reads), [0], 1), reads=reads, counts=counts if counts is not None else
                np.arange(1, len(reads) + 1, dtype=np.uint32), entry_keep=None, n_entries=1, threshold=t)


def acgt(rng, L):
    return "".join("ACGT"[c] for c in rng.integers(0, 4, L))


# ------------------------------------------------------------------------------------------------ threshold edges
@pytest.mark.parametrize("t", [1, 14, 15])
def test_threshold_edges(stages, t):
    """cluster_heads_kernel's `s <= P && P - s + 1 >= t` at overlaps t - 1, t, t + 1, s = E and s = E + 1, and
    cluster_assemble_kernel's `e <= P` for rows ending at or before E; equal keys keep read order."""
    rng = np.random.default_rng(t)
    reads = [acgt(rng, L) for L in (25, 30, 22, 10, 20, 16, 28)]
    rows, at = [], 0

    def pile(*more):        # a 25-nt head at `at`, E = at + 25; the others are placed by their overlap with it
        nonlocal at
        rows.append((0, at))
        for r, overlap in more:
            rows.append((r, at + 25 - overlap))
        at += 1000

    for o in (t - 1, t, t + 1):
        pile((1, o))
        pile((3, o), (2, o))                   # the same from two reads at one position, of 22 and 10 nt
    pile((1, 1))                               # s = E
    pile((1, 0))                               # s = E + 1
    pile((3, 10))                              # e = E from a 10-nt read
    pile((4, 20))                              # e = E from a 20-nt read
    pile((5, 18))                              # e < E
    pile((1, 15), (1, 15))                     # two identical rows
    rows += [(6, at), (2, at), (4, at)]        # three reads at one position: the members are 2, 4, 6
    at += 1000
    rows += [(5, at), (5, at), (5, at)]        # ... and three times the same row
    got, want = check(stages, one_list(rows[::-1], reads, t))
    assert want["n_clusters"] >= 14
    i = want["rows_cluster"][2].tolist().index(at - 1000)
    assert got["rows_cluster"][0][i:i + 3].tolist() == [2, 4, 6]


# ------------------------------------------------------------------------------------------------ running maximum
def running_max_rows():
    rng = np.random.default_rng(5)
    reads = [acgt(rng, 200), acgt(rng, 5), acgt(rng, 30), acgt(rng, 30)] + [acgt(rng, L) for L in range(1, 14)]
    rows = [(0, 0)]
    rows += [(4 + k, 5 + 11 * k) for k in range(13)] + [(4 + k, 150 + k) for k in range(13)]     # contained, 1..13 nt
    rows += [(2, 180)]          # [181, 210]: 20 bases of [1, 200], none of the short reads in front of it
    rows += [(1, 200)]          # [201, 205]: 10 bases of [1, 210]: a cluster of its own that ends before 210
    rows += [(3, 203)]          # [204, 233]: 7 bases of [1, 210], 2 of [201, 205]: the next cluster
    rows += [(4 + k, 1000 + 3 * k) for k in range(13)] + [(4 + k, 1000 + 3 * k) for k in range(0, 13, 2)]   # 1..13 nt alone at t = 14
    rows += [(16, 2000), (10, 2000), (5, 2001)]       # 13 nt, then 7 nt and 2 nt inside it: 13 bases are not enough
    return one_list(rows, reads, 14)


def test_long_read_then_contained_short_reads(stages):
    """cluster_heads_kernel reads P = runmax[i - 1], not the row in front: short reads inside a 200-nt read, a row that
    joins only through the long read's end, a single-row cluster that ends before P (cluster_bounds_kernel's
    `j - i == 1 ? w.end[i]`), reads of 1..13 nt at t = 14."""
    kw = running_max_rows()
    got, want = check(stages, kw)
    # the input has the structure: the row in front of the joining one ends more than t bases before it ...
    read, _, pos, _, _ = (x.tolist() for x in want["rows_cluster"])
    i = read.index(2)
    assert pos[i] == 180 and pos[i - 1] + len(kw["reads"][read[i - 1]]) < 181 + 13
    # ... the first cluster ends at 210, the single row [201, 205] is the second, [204, 233] opens the third
    assert want["member_off"][1] > 20 and want["end"][0] == 210 and (want["end"][1], want["start"][2]) == (205, 204)
    assert want["n_clusters"] > 20


# ------------------------------------------------------------------------------------------------ lists
def test_lists_by_entry_and_strand(stages):
    """cluster_rows_kernel's list head `(kp >> pos_bits) != (k >> pos_bits)`: the same entry on + then -, one position
    on both strands, a new entry; cluster_keys_kernel's kSamOrder key puts + before - at one position."""
    rng = np.random.default_rng(8)
    reads = [acgt(rng, L) for L in (24, 24, 30, 18, 40)]
    rows = []
    for e in range(3):
        for s in (1, 0):
            rows += [(r, e, 100 + 4 * r, s, r % 3) for r in range(5)]       # the same piles on every list: no row joins across
        rows += [(4, e, 100, 1, 0), (3, e, 100, 0, 1)]
    kw = dict(parts=model.make_parts(rows, 5, [0, 2], 3), reads=reads, counts=np.arange(1, 6, dtype=np.uint32), entry_keep=None,
              n_entries=3, threshold=14)
    got, want = check(stages, kw)
    assert want["n_clusters"] == 6 and want["strand"].tolist() == [0, 1] * 3
    sam = got["rows_sam"]
    at100 = [(int(e), int(s), int(r)) for r, e, p, s, _ in zip(*sam) if p == 100]
    assert at100[:4] == [(0, 0, 0), (0, 0, 3), (0, 1, 0), (0, 1, 4)]


# ------------------------------------------------------------------------------------------------ mask
def mask_rows(seed=3, rows_per_entry=40):
    return model.random_rows(np.random.default_rng(seed), 5 * rows_per_entry, 14, max_len=40, n_entries=5, n_parts=2, masked=0)


@pytest.mark.parametrize("keep", ["first", "middle", "last", "all", "null", "two"])
def test_entry_mask(stages, keep):
    """cluster_keys_kernel's `e = n_entries` for a masked entry and the one writer of *w.n_valid in cluster_rows_kernel:
    the first, a middle, the last or every entry masked, and no mask.  Masked rows keep their entry under MRG_SAM_ORDER."""
    kw = mask_rows()
    flags = {"first": [0, 1, 1, 1, 1], "middle": [1, 1, 0, 1, 1], "last": [1, 1, 1, 1, 0], "all": [0] * 5, "two": [1, 0, 1, 0, 1],
             "null": None}[keep]
    kw["entry_keep"] = None if flags is None else np.array(flags, np.uint8)
    got, want = check(stages, kw, keep)
    if keep == "all":
        assert (got["n_valid"], got["n_clusters"], got["total_len"]) == (0, 0, 0)
        assert got["member_off"].tolist() == [0] and got["len"].tolist() == [0] and got["seq_off"].tolist() == [0]
    elif keep != "null":
        assert 0 < got["n_valid"] < got["n_rows"]
        assert set(got["rows_cluster"][1][got["n_valid"]:].tolist()) == {5}
        assert set(got["rows_sam"][1].tolist()) == {0, 1, 2, 3, 4}


@pytest.mark.parametrize("valid", [0, 1, 255, 256, 257])
def test_mask_boundary_at_a_block_edge(stages, valid):
    """cluster_rows_kernel's `!valid && prev_valid` at sorted row 0, 255, 256, 257: the thread that writes n_valid is
    the first of a block, the last of one, or has no row in front of it."""
    rng = np.random.default_rng(valid)
    reads = [acgt(rng, int(L)) for L in rng.integers(5, 40, 50)]
    rows = [(int(rng.integers(0, 50)), 1, int(rng.integers(0, 2000)), int(rng.integers(0, 2)), 0) for _ in range(valid)]
    rows += [(int(rng.integers(0, 50)), int(e), int(rng.integers(0, 2000)), int(rng.integers(0, 2)), 1) for e in rng.choice([0, 2], 300)]
    kw = dict(parts=model.make_parts(rows, 50, [0], 3), reads=reads, counts=np.arange(50, dtype=np.uint32), n_entries=3,
              entry_keep=np.array([0, 1, 0], np.uint8), threshold=14)
    got, _ = check(stages, kw)
    assert got["n_valid"] == valid and got["n_rows"] == valid + 300


# ------------------------------------------------------------------------------------------------ parts and owners
def test_parts_row_base_and_empty_reads(stages):
    """cluster_keys_kernel's binary search over `offsets` and its `row_base + k` / `entry_base + ref`: three parts, the
    middle one without rows, reads without rows in front, inside and behind."""
    rng = np.random.default_rng(12)
    n = 12
    reads = [acgt(rng, int(L)) for L in rng.integers(10, 60, n)]
    owners = [2, 3, 3, 3, 5, 8, 8, 9]                           # reads 0, 1, 4, 6, 7, 10, 11 own nothing
    rows = [(r, int(e), int(rng.integers(0, 300)), int(rng.integers(0, 2)), int(rng.integers(0, 3)))
            for e in (0, 1, 5, 6) for r in owners for _ in range(2)]
    kw = dict(parts=model.make_parts(rows, n, [0, 2, 5], 7), reads=reads, counts=rng.integers(1, 100, n).astype(np.uint32),
              entry_keep=np.array([1, 1, 1, 1, 1, 0, 1], np.uint8), n_entries=7, threshold=14)
    assert [len(p["ref"]) for p in kw["parts"]] == [32, 0, 32] and kw["parts"][2]["ref"].max() == 1
    got, want = check(stages, kw)
    assert set(want["entry"].tolist()) == {0, 1, 6}


def test_one_read_owns_every_row(stages):
    """cluster_keys_kernel's search when one interval holds all rows: the first, a middle and the last read."""
    rng = np.random.default_rng(13)
    reads = [acgt(rng, 21), acgt(rng, 34), acgt(rng, 27)]
    for r in range(3):
        rows = [(r, int(e), int(p), int(s), 0) for e, p, s in zip(rng.integers(0, 2, 300), rng.integers(0, 600, 300), rng.integers(0, 2, 300))]
        kw = dict(parts=model.make_parts(rows, 3, [0], 2), reads=reads, counts=[4, 5, 6], entry_keep=None, n_entries=2, threshold=14)
        got, _ = check(stages, kw, "read %d" % r)
        assert set(got["member_all"].tolist()) == {r}


# ------------------------------------------------------------------------------------------------ words
LENGTHS = (1, 31, 32, 33, 63, 64, 65, 128, 129, 255)
N_AT = (0, 31, 32, 63, 64)
TAIL_FROM = (1, 31, 32, 33, 64)


def word_rows(W, with_n):
    """Per read length that fits W words and per strand: the read alone, and as the row that joins a cluster with
    P - s + 1 in TAIL_FROM + (L - 1,) -- each in an entry of its own, threshold 1.  Two reads per length, one with N at
    N_AT + (L - 1,)."""
    rng = np.random.default_rng(100 + W)
    reads, rows, entry = [], [], 0
    heads = {}

    def head_of(L):          # a head read of L nt, shared
        if L not in heads:
            heads[L] = len(reads)
            reads.append(acgt(rng, L))
        return heads[L]

    for L in (x for x in LENGTHS if x <= 32 * W):
        plain, marked = acgt(rng, L), list(acgt(rng, L))
        for q in N_AT + (L - 1,):
            if q < L and with_n:
                marked[q] = "N"
        # (head length, from): the joiner has `from` bases of the head; the heads get the lower read numbers, so that a
        # head as long as `from` still comes first at the position it then shares with the joiner
        tails = [(frm + 7 if frm + 7 <= 32 * W else frm, frm) for frm in sorted(set(TAIL_FROM + (L - 1,))) if 1 <= frm < L]
        tails = [(head_of(LH), LH, frm) for LH, frm in tails]
        mine = (len(reads), len(reads) + 1)
        reads += [plain, "".join(marked)]
        for strand in (0, 1):
            for r in mine:
                rows.append((r, entry, 7, strand, 0))
                entry += 1
                for head, LH, frm in tails:
                    rows.append((head, entry, 10, strand, 1))
                    rows.append((r, entry, 10 + LH - frm, strand, 2))
                    entry += 1
    return dict(parts=model.make_parts(rows, len(reads), [0, entry // 2], entry), reads=reads,
                counts=np.arange(1, len(reads) + 1, dtype=np.uint32), entry_keep=None, n_entries=entry, threshold=1)


@pytest.mark.parametrize("mask", ["present", "null"])
@pytest.mark.parametrize("W", [1, 2, 4, 8])
def test_every_word_of_a_read(stages, W, mask):
    """cluster_assemble_kernel's reload of `word` / `nm` when `q >> 5` changes, `q = L - 1 - j` and `3 - code` on the -
    strand, the N bit of the higher mask words, `from = P - s + 1` at and around the word boundaries, garbage behind the
    last base; with the mask and with nmask = NULL (then no read has an N)."""
    kw = word_rows(W, with_n=(mask == "present"))
    got, want = check(stages, kw, W=W, nmask=mask, garbage=True)
    assert got["W"] == W
    two = np.flatnonzero(np.diff(want["member_off"].astype(np.int64)) == 2)
    assert want["n_clusters"] == kw["n_entries"] and two.size > want["n_clusters"] // 2
    assert (b"N" in want["seq"]) == (mask == "present")
    if W == 8:
        assert int(want["len"].max()) >= 255 + 7


# ------------------------------------------------------------------------------------------------ sums
def test_sums_are_64_bit(stages):
    """cluster_assemble_kernel's atomicAdd on a 64-bit sum: three members of 2^32 - 1 copies in one cluster, and a read
    that is a member of two clusters."""
    rng = np.random.default_rng(21)
    reads = [acgt(rng, 22) for _ in range(5)]
    big = 2 ** 32 - 1
    rows = [(0, 100), (1, 102), (2, 104), (3, 105), (3, 5000), (4, 5003), (0, 5004)]
    kw = one_list(rows, reads, 14, counts=np.array([big, big, big, 11, 5], np.uint32))
    got, want = check(stages, kw)
    assert want["sum"] == [3 * big + 11, 11 + 5 + big] and got["sum"][0] > 2 ** 33


# ------------------------------------------------------------------------------------------------ key range
def test_one_position_bit(stages):
    """pos_bits = 1: the strand bit is bit 1 of the key, the entry starts at bit 2."""
    rng = np.random.default_rng(31)
    reads = [acgt(rng, int(L)) for L in rng.integers(1, 30, 20)]
    rows = [(int(r), int(e), int(p), int(s), 0) for r, e, p, s in zip(rng.integers(0, 20, 200), rng.integers(0, 6, 200),
                                                                       rng.integers(0, 2, 200), rng.integers(0, 2, 200))]
    kw = dict(parts=model.make_parts(rows, 20, [0, 3], 6), reads=reads, counts=np.arange(20, dtype=np.uint32),
              entry_keep=np.array([1, 1, 0, 1, 1, 1], np.uint8), n_entries=6, threshold=2)
    check(stages, kw, pos_bits=1)


def test_widest_key(stages):
    """pos_bits = 31, n_entries = 2^32 - 2 without a mask, rows on the entries 0 and 2^32 - 3, at the offsets 0 and
    2^31 - 1 - L: all 64 key bits are sorted, `e << (pos_bits + 1)` and the 32-bit end `pos + len` are at their limits."""
    rng = np.random.default_rng(32)
    lens = [255, 30, 1, 64, 20]
    reads = [acgt(rng, L) for L in lens]
    top = 2 ** 32 - 3
    rows = []
    for e in (0, top):
        for s in (0, 1):
            rows += [(r, e, 2 ** 31 - 1 - L, s, 1) for r, L in enumerate(lens)] + [(r, e, 0, s, 2) for r in range(5)]
            rows += [(1, e, 2 ** 31 - 1 - 40, s, 0), (4, e, 2 ** 31 - 1 - 255, s, 0)]
    rows = [rows[i] for i in rng.permutation(len(rows))]
    rows.sort(key=lambda r: r[0])
    parts = model.make_parts(rows, 5, [0, top], 2 ** 32 - 2)
    assert parts[1]["entry_base"] == top and (parts[1]["ref"] == 0).all()
    kw = dict(parts=parts, reads=reads, counts=np.arange(1, 6, dtype=np.uint32), entry_keep=None, n_entries=2 ** 32 - 2, threshold=14)
    got, want = check(stages, kw, pos_bits=31)
    assert int(want["end"].max()) == 2 ** 31 - 1 and set(want["entry"].tolist()) == {0, top}


# ------------------------------------------------------------------------------------------------ sizes
@pytest.mark.parametrize("rows", [1, 255, 256, 257, 4095, 4096, 4097, 8193, 65537])
def test_row_counts_across_blocks_and_tiles(stages, rows):
    """Every kernel's `i >= rows` / `i >= n_valid` guard and the primitives' tiles: row counts around the 256-thread
    block and the 4096-element tile, and 65 537."""
    rng = np.random.default_rng(rows)
    kw = model.random_rows(rng, rows, 14, max_len=int(rng.choice([32, 64, 128])), n_entries=4, n_parts=2, masked=rows % 2)
    got, want = check(stages, kw, garbage=True)
    assert got["n_rows"] == rows


def test_a_list_longer_than_two_tiles_under_one_long_read(stages):
    """prims::segmented_inclusive_max_u32 as cluster_heads_kernel and cluster_assemble_kernel use it: a 255-nt read
    opens a list of 9000 rows of 1..13 nt that lie inside it, so its end is the carried maximum of three tiles; the
    rows behind offset 241 have fewer than 14 bases of it and are clusters of their own that end before P, and a chain
    of 30-nt reads goes on from offset 250."""
    rng = np.random.default_rng(41)
    reads = [acgt(rng, 255)] + [acgt(rng, 1 + k % 13) for k in range(40)] + [acgt(rng, 30) for _ in range(20)]
    rows = [(0, 0)]
    for _ in range(9000):
        r = int(rng.integers(1, 41))
        rows.append((r, int(rng.integers(0, 256 - len(reads[r])))))
    rows += [(41 + k, 250 + 9 * k) for k in range(20)]
    rows = [rows[i] for i in rng.permutation(len(rows))]
    got, want = check(stages, one_list(rows, reads, 14))
    n_members = np.diff(want["member_off"].astype(np.int64))
    assert n_members[0] > 8192 and want["end"][0] == 255 and (n_members == 1).sum() > 50 and n_members[-1] >= 20


def test_one_cluster_of_five_thousand_members(stages):
    """cluster_bounds_kernel's walk `while (j < n_valid && !chead[j])` over more than a tile and its `runmax[j - 1]`:
    5000 rows of 20..40 nt, each two bases on, on both strands: 5000 writers of a few bases each to one sequence."""
    rng = np.random.default_rng(42)
    reads = [acgt(rng, int(L)) for L in rng.integers(20, 41, 64)]
    rows = [(int(rng.integers(0, 64)), 2 * i, s) for s in (0, 1) for i in range(5000)]
    rows += [(3, 10000 + 41), (4, 10000 + 41, 1)]                # behind the last end: the walk stops at a head
    got, want = check(stages, one_list(rows, reads, 14))
    assert np.diff(want["member_off"].astype(np.int64)).tolist() == [5000, 1, 5000, 1]


# ------------------------------------------------------------------------------------------------ random
@pytest.mark.parametrize("seed", range(24))
def test_random_rows(stages, seed):
    """All stages on the generator's mix of duplicates, shared positions, contained and abutting rows, overlaps around
    the threshold and reads below it; W and t drawn per seed."""
    rng = np.random.default_rng(7000 + seed)
    t = (1, 5, 14, 15, 40)[seed % 5]
    max_len = (32, 64, 128, 255)[(seed // 5) % 4]
    kw = model.random_rows(rng, int(rng.integers(200, 5001)), t, max_len=max_len, n_entries=int(rng.integers(2, 9)),
                           n_parts=int(rng.integers(1, 4)), masked=int(rng.integers(0, 2)), max_count=2 ** 32 - 1)
    null = seed % 3 == 0            # every third seed without an N and without a mask
    if null:
        kw["reads"] = [s.replace("N", "A") for s in kw["reads"]]
    check(stages, kw, "seed %d" % seed, W=(1, 2, 4, 8)[(seed // 5) % 4], nmask="null" if null else "present", garbage=seed % 2 == 1)


# ------------------------------------------------------------------------------------------------ through the engine
def small_world(seed=77):
    """Two parts of two entries (one not a chromosome), 360 distinct reads of 33..70 nt cut from loci on both strands,
    every ninth with an N behind the 25-nt seed."""
    rng = np.random.default_rng(seed)
    names = ["chr1", "chr2", "scaffold_3", "chr4"]
    texts = [acgt(rng, 4000) for _ in names]
    comp = str.maketrans("ACGT", "TGCA")
    loci = [(int(rng.integers(0, 4)), int(rng.integers(100, 3800))) for _ in range(40)]
    seqs = []
    while len(seqs) < 360:
        e, at = loci[int(rng.integers(0, len(loci)))]
        at += int(rng.integers(-30, 31))
        q = texts[e][at:at + int(rng.integers(33, 71))]
        if rng.integers(0, 2):
            q = q[::-1].translate(comp)
        if len(seqs) % 9 == 4:
            k = int(rng.integers(26, len(q)))
            q = q[:k] + "N" + q[k + 1:]
        if q not in seqs:
            seqs.append(q)
    return names, texts, seqs


def test_engine_cluster_valid_on_two_word_reads(native_lib, tmp_path):
    """Engine.cluster_valid against the model fed with Engine.list_valid's rows of the same reads and policy: only the
    clustering is under test.  The reads need two words, and a - strand row must join with a tail whose first base lies
    in word 1 (cluster_assemble_kernel's `q = L - 1 - j` walking down across a word)."""
    from mirge_amd import pack, predict
    from mirge_amd.engine import Engine, ReadSet, STRATUM_ALL
    from mirge_amd.index import FmIndex
    names, texts, seqs = small_world()
    for k in range(2):
        FmIndex.build(names[2 * k:2 * k + 2], texts[2 * k:2 * k + 2]).save("%s.part%03d.mrgfm" % (tmp_path / "g", k))
    eng = Engine(0)
    try:
        keys, parts = predict.genome_libraries(eng, str(tmp_path / "g"))
        words, lens, nmask = pack.pack_reads(seqs)
        rs = ReadSet(words, lens, nmask, device=eng.device)
        assert rs.W >= 2 and nmask is not None
        counts = np.random.default_rng(1).integers(1, 2 ** 32, len(seqs)).astype(np.uint32)
        keep = np.array(["chr" in n for n in names])
        policy = dict(strands=2, stratum_mode=STRATUM_ALL, m=3, seed_len=25, max_mm_seed=0, max_mm_total=2)
        t = 14
        off, entry, pos, strand, mm, supp = eng.list_valid(rs, keys, **policy)
        got = eng.cluster_valid(rs, keys, counts, entry_keep=keep, threshold=t, sorted_rows=True, **policy)
    finally:
        eng.close()
    part = dict(offsets=off.astype(np.uint64), ref=entry, pos=pos, strand=strand, mm=mm, entry_base=0)
    want = model.cluster_rows([part], seqs, counts, keep, len(names), t)
    assert want["n_rows"] > 300 and 0 < want["n_valid"] < want["n_rows"] and np.array_equal(supp, got["suppressed"])
    assert (got["n_rows"], got["n_valid"], len(got["entry"])) == (want["n_rows"], want["n_valid"], want["n_clusters"])
    for name, wname in (("entry", "entry"), ("strand", "strand"), ("start", "start"), ("end", "end"), ("seq_off", "seq_off"),
                        ("member_off", "member_off"), ("members", "member")):
        assert np.array_equal(got[name], want[wname]), "%s: %s" % (name, first_diff(got[name], want[wname]))
    assert got["seq"] == want["seq"] and b"N" in want["seq"]
    assert [int(x) for x in got["count_sum"]] == want["sum"] and max(want["sum"]) > 2 ** 32
    for name, g, w in zip(("read", "entry", "offset", "strand", "mm"), got["rows"], want["rows_sam"]):
        assert np.array_equal(g, w), "sorted rows %s: %s" % (name, first_diff(g, w))
    # the path this test is for: a joining - strand row whose tail SEQ[from:] starts at read base L - 1 - from >= 32
    read, _, rpos, rstrand, _ = (x.tolist() for x in want["rows_cluster"])
    deep = 0
    for c in np.flatnonzero(want["strand"] == 1).tolist():
        E = None
        for i in range(int(want["member_off"][c]), int(want["member_off"][c + 1])):
            s, L = rpos[i] + 1, len(seqs[read[i]])
            if E is not None and s + L - 1 > E and L - 1 - (E - s + 1) >= 32:
                deep += 1
            E = max(E or 0, s + L - 1)
    assert deep > 0, "no - strand tail reaches into word 1: the world no longer exercises the path"
