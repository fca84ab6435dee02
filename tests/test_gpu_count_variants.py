"""count_variants_kernel (csrc/kernels.hip; the `-ai` genome filter, W2C:1251-1287) against the exhaustive scan, class
by class.

The kernel is a case analysis: with K = the largest jump table's k <= L, an alignment with at most one mismatch belongs to
A (first K bases exact), to B (last K exact, the mismatch in front of base L - K) or to one variant per (position in
[L - K, K), other base).  A mistake at a class boundary counts an alignment twice or drops it, so every read here is
compared as (best_mm, count) == oracle.model.best_stratum -- the scan of the library strings, no index -- exactly, on
one-word reads without N (the only ones mrg_count_best gives to this kernel), once with the default options and once
with count_kernel alone (`count_variants` = 0); `count_variants` = 2 runs the variants kernel ALONE and shows which
reads it answered.

Libraries of a few kb reach the kernel's real work because every library gets jump tables {4, 6, k_mid >= 8, k_big}
(plan_jump_tables): S (12 kb) has k = 8, 9; M (300 kb) has k = 10, 11, the miniature of a genome part's K = 14 with
L = 18..21.  Exactness needs that no lookup is cut short at 4096 rows: asserted from the strings before any GPU call.

What the file was seen to notice (one-line changes to count_variants_kernel, each built and run once): without the
`it == 1 && first mismatch >= K` line, the class-boundary tests on S fail for L = 19..28 (L > 2K counted twice); with the
variants started at tail + 1, those on S for L = 8..17 and on M for L = 10..21; with the table loop keeping the first table
that fits, only test_variants_kernel_alone_... and the `count_variants` = 2 run of the grid-stride test (count_kernel
answers every read, rightly).  Dropping `it != 0 && mm != 1` changes nothing: a variant's K-mer differs from the read, so
it never sees mm == 0, and B's exact hit is skipped by the first-mismatch line too (ffs(0) - 1 wraps to a position >= K).
"""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from oracle import model

pytestmark = pytest.mark.gpu

POLICIES = [(28, 1, 2), (28, 1, 1), (20, 1, 1), (32, 1, 2)]   # (seed_len, max_mm_seed, max_mm_total); the first is a2i's
MAX_ROWS = 4096        # capi.hip: fill_count_params
TODO = 254             # kernels.hip: kCountTodoMark
S_LENGTHS = list(range(8, 29))
M_LENGTHS = list(range(10, 23))
# substitutions of the planted copies of a 32-base unit: a site WITH the unchanged copy (first third / middle / last third),
# and the two sites WITHOUT it, whose reads have a best stratum of 1 with hits owned by different classes
SITE_EXACT = (None, 5, 16, 27)
SITE_X = (12, 16, 20)
SITE_Y = (6, 15, 25)


def _rnd(rng, n):
    return np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n)].tobytes().decode()


def _sub(s, p, k):
    """s with base p replaced by the k-th (0..2) of the three other bases."""
    return s[:p] + [c for c in "ACGT" if c != s[p]][k] + s[p + 1:]


def _max_kmer_rows(seqs, k):
    """Most rows a k-mer lookup can meet: occurrences of the commonest k-mer of the concatenated entries (a k-mer that
    runs over an entry's end has rows in the jump table too; an N breaks a k-mer)."""
    code = np.full(256, 4, dtype=np.int64)
    code[np.frombuffer(b"ACGT", dtype=np.uint8)] = np.arange(4)
    c = code[np.frombuffer("".join(seqs).encode("ascii"), dtype=np.uint8)]
    n = c.size - k + 1
    key, bad = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=bool)
    for i in range(k):
        key = key * 4 + (c[i:i + n] & 3)
        bad |= c[i:i + n] > 3
    return int(np.unique(key[~bad], return_counts=True)[1].max())


class _World:
    """One library: its strings, the scan's view of it, its index on the engine, and the scan's answers so far."""

    def __init__(self, eng, key, names, seqs, sites=None):
        from mirge_amd.index import FmIndex
        self.eng, self.key, self.names, self.seqs, self.sites = eng, key, names, seqs, sites or {}
        self.olib = model.Library(names, seqs)
        self.ix = FmIndex.build(names, seqs)
        self.ks = [int(k) for k in self.ix.info.ftab_ks]
        eng.add_library(key, self.ix)
        self.memo = {}

    def table_k(self, L):
        """The kernel's K for a read of L bases: the largest jump table's k <= L (0: none)."""
        return max([k for k in self.ks if k and k <= L], default=0)

    def expect(self, reads, policy):
        """[(em, min(ec, 255))] by exhaustive scan.  The scan reads seed_len only as min(len, seed_len)
        (oracle/bowtie_model.c: orc_best_stratum), so that is what an answer is remembered under."""
        seed_len, mms, mmt = policy
        keys = [(r, min(len(r), seed_len), mms, mmt) for r in reads]
        todo = [k for k in dict.fromkeys(keys) if k not in self.memo]
        if todo:
            with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:   # (the scan runs outside the GIL)
                got = list(pool.map(lambda k: model.best_stratum(self.olib, k[0], seed_len, mms, mmt), todo, chunksize=16))
            for k, (em, ec) in zip(todo, got):
                self.memo[k] = (em, min(ec, 255), ec)
        return [self.memo[k][:2] for k in keys]

    def scan_count(self, read, policy):
        self.expect([read], policy)
        return self.memo[(read, min(len(read), policy[0]), policy[1], policy[2])][2]


def _planted(rng, lens, n_exact_sites):
    """Random entries of the given lengths with planted sites: each a random unit of 32 bases written into different
    entries, once per element of its substitution tuple (None = unchanged)."""
    seqs = [list(_rnd(rng, n)) for n in lens]
    big = [e for e, n in enumerate(lens) if n >= 500]
    slot = {e: 0 for e in big}
    sites, turn = {}, 0
    plan = [("exact%d" % i, SITE_EXACT) for i in range(n_exact_sites)] + [("x", SITE_X), ("y", SITE_Y)]
    for name, subs in plan:
        unit = _rnd(rng, 32)
        for p in subs:
            e = big[turn % len(big)]
            turn += 1
            at = 96 + 48 * slot[e]
            slot[e] += 1
            assert at + 32 <= lens[e] - 40
            seqs[e][at:at + 32] = list(unit if p is None else _sub(unit, p, 1))
        sites[name] = unit
    return ["".join(s) for s in seqs], sites


@pytest.fixture(scope="module")
def engine(native_lib, oracle_lib):
    from mirge_amd.engine import Engine
    return Engine(0)


@pytest.fixture(scope="module")
def world_s(engine):
    """S: 12 kb in a dozen entries (tables k = 9, 8, 6, 4), an entry of 17 bases, one library N, planted sites."""
    rng = np.random.default_rng(901)
    lens = [1400, 900, 17, 1300, 800, 1200, 600, 1100, 1000, 1500, 700, 1483]
    seqs, sites = _planted(rng, lens, 2)
    seqs[4] = seqs[4][:60] + "N" + seqs[4][61:]
    assert max(_max_kmer_rows(seqs, k) for k in (8, 9)) <= MAX_ROWS      # no lookup is cut short: equality is exact
    w = _World(engine, "S", ["s%d" % i for i in range(len(seqs))], seqs, sites)
    assert w.ks == [9, 8, 6, 4]
    return w


@pytest.fixture(scope="module")
def world_m(engine):
    """M: 300 kb, 4^9 < n <= 4^10 (tables k = 11, 10, 6, 4): a genome part's K = 14, L = 18..21 in miniature."""
    rng = np.random.default_rng(902)
    seqs, sites = _planted(rng, [30000] * 10, 2)
    assert 4 ** 9 < sum(len(s) for s in seqs) <= 4 ** 10
    assert max(_max_kmer_rows(seqs, k) for k in (10, 11)) <= MAX_ROWS
    w = _World(engine, "M", ["m%d" % i for i in range(len(seqs))], seqs, sites)
    assert w.ks == [11, 10, 6, 4]
    return w


def _x_origin(L):
    """Where a read of L bases is cut from site x: its middle substitution near the read's middle (between the class
    boundaries L - K and K), all three inside the read where L allows it."""
    return min(max(16 - L // 2, 0, 21 - L), 12, 32 - L)


def _origins(world, L, seed):
    """Reads of L bases to start from: cut from a site with the unchanged copy, from the two sites without it (placed so
    that their copies' substitutions fall on both sides of the class boundaries), and from a random place."""
    rng = np.random.default_rng(seed * 1000 + L)
    s = world.sites
    out = [s["exact%d" % (L & 1)][(32 - L) // 2:][:L]]
    o = _x_origin(L)
    out.append(s["x"][o:o + L])
    if L >= 20:
        o = min(6, 32 - L)
        out.append(s["y"][o:o + L])
    e = int(rng.choice([i for i, q in enumerate(world.seqs) if len(q) >= 500 and "N" not in q]))
    o = int(rng.integers(0, len(world.seqs[e]) - L))
    out.append(world.seqs[e][o:o + L])
    return out


def _boundary_reads(world, L, seed=1):
    """Case set (a) for one read length: per origin the read itself, one substitution at EVERY position (all three other
    bases at the class boundaries L-K-1, L-K, K-1, K), and reads with two substitutions, one in each half."""
    K = world.table_k(L)
    reads = []
    for base in _origins(world, L, seed):
        reads.append(base)
        reads += [_sub(base, p, (p + L) % 3) for p in range(L)]
        for p in sorted({L - K - 1, L - K, K - 1, K}):
            if 0 <= p < L:
                reads += [_sub(base, p, k) for k in range(3)]
        for p, q in ((0, L - 1), (L // 2 - 1, L // 2), (L // 4, L - 1 - L // 4)):
            reads.append(_sub(_sub(base, p, 1), q, 2))
    return reads


def _read_set(eng, reads):
    from mirge_amd import pack
    from mirge_amd.engine import ReadSet
    words, lens, nmask = pack.pack_reads(reads)
    assert words.shape[0] == 1 and nmask is None        # else mrg_count_best does not launch the variants kernel
    return ReadSet(words, lens, None, None, device=eng.device)


def _run(world, rs, policy, variants):
    world.eng.set_option("count_variants", variants)
    try:
        mm, cnt = world.eng.count_best(rs, world.key, seed_len=policy[0], max_mm_seed=policy[1], max_mm_total=policy[2])
    finally:
        world.eng.set_option("count_variants", 1)
    return list(zip(mm.tolist(), cnt.tolist()))


def _check(world, reads, policies=POLICIES):
    """Both kernels' answers for the batch = the scan's, under every policy; returns the scan's answers per policy."""
    rs = _read_set(world.eng, reads)
    wants = {}
    for policy in policies:
        want = wants[policy] = world.expect(reads, policy)
        for variants in (1, 0):
            got = _run(world, rs, policy, variants)
            bad = [i for i in range(len(reads)) if got[i] != want[i]]
            assert not bad, ("%d of %d reads differ from the scan" % (len(bad), len(reads)), world.key, policy,
                             "count_variants=%d" % variants,
                             [(reads[i], "got", got[i], "scan", want[i]) for i in bad[:6]])
    return wants


def _quiet(world, L):
    """True where chance hits are out of reach: a random L-mer has fewer than 0.01 places with at most one mismatch in
    this library, so that what a planted read must give can be asserted on top of its equality with the scan."""
    return sum(len(s) for s in world.seqs) * (1 + 3 * L) / 4.0 ** L < 0.01


def _assert_strata(want, L):
    """The batch of one length holds exact, one-mismatch and unalignable reads in numbers (not only equal answers)."""
    assert sum(w[0] == 0 for w in want) >= 3 and sum(w[0] == 1 for w in want) >= 2 * L and sum(w[0] == 255 for w in want) >= 3


def _class_of(world, L, p):
    K = world.table_k(L)
    return "A" if p >= K else ("B" if p < L - K else "variant")


@pytest.mark.parametrize("L", S_LENGTHS)
def test_class_boundaries_on_s(world_s, L):
    """(a) on S: K = 8 for L = 8 (L == K: B is A), K = 9 above -- variants for L < 18, none at L == 2K = 18, and from
    L = 19 on A and B do not meet: a mismatch between them leaves both exact and is A's."""
    reads = _boundary_reads(world_s, L)
    want = _check(world_s, reads)[POLICIES[0]]
    if _quiet(world_s, L):      # (L >= 13) the read cut from site x: three one-mismatch hits and no exact one
        _assert_strata(want, L)
        assert world_s.expect([_origins(world_s, L, 1)[1]], POLICIES[0]) == [(1, 3)]


@pytest.mark.parametrize("L", M_LENGTHS)
def test_class_boundaries_on_m(world_m, L):
    """(a) on M: K = 10 for L = 10, K = 11 above, so L = 18..21 have 3 * (4..1) variants as a genome part's reads have;
    the reads cut from the sites without an unchanged copy have hits in different classes."""
    reads = _boundary_reads(world_m, L)
    want = _check(world_m, reads)[POLICIES[0]]
    o = _x_origin(L)
    if L >= 14:                 # site x's three copies differ from its read in different classes
        assert len({_class_of(world_m, L, p - o) for p in SITE_X}) >= 2
    if _quiet(world_m, L):      # (L >= 16) ... and they are all the read has: stratum 1, three hits, no exact one
        _assert_strata(want, L)
        assert world_m.expect([_origins(world_m, L, 1)[1]], POLICIES[0]) == [(1, 3)]
    if L == 20:
        assert {_class_of(world_m, L, p - 6) for p in SITE_Y} == {"A", "B", "variant"}
        assert world_m.expect([_origins(world_m, L, 1)[2]], POLICIES[0]) == [(1, 3)]


def _handover_extras(world, rng):
    """Reads count_variants_kernel must leave to count_kernel: shorter than a usable table (1, 2, 4, 7 nt), longer than
    the seed (29..32 nt under seed_len 28, 21..30 under 20).  -> (reads, indices of the 29..32-nt reads whose single
    substitution lies behind base 28)."""
    long_entries = [i for i, q in enumerate(world.seqs) if len(q) >= 500 and "N" not in q]

    def window(L):
        e = int(rng.choice(long_entries))
        o = int(rng.integers(0, len(world.seqs[e]) - L))
        return world.seqs[e][o:o + L]
    reads, behind = list("ACGT"), []
    for L, subs in ((2, (0,)), (4, (1,)), (7, (0, 3, 6))):
        for _ in range(2):
            b = window(L)
            reads += [b] + [_sub(b, p, 2) for p in subs]
    for L in range(29, 33):
        for b in (window(L), window(L), world.sites["exact0"][:L]):
            reads.append(b)
            for p in (0, 13, 27, 28, L - 1):
                if p >= 28:
                    behind.append(len(reads))
                reads.append(_sub(b, p, p % 3))
            reads += [_sub(_sub(b, 5, 0), L - 1, 1), _sub(_sub(b, 3, 0), 20, 1)]
    for L in range(21, 29):
        for b in (window(L), world.sites["exact1"][2:2 + L]):
            reads += [b] + [_sub(b, p, p % 3) for p in (2, 19, 20, L - 1)] + [_sub(_sub(b, 4, 0), L - 1, 1)]
    return reads, behind


def _handover_batch(world):
    rng = np.random.default_rng(903)
    extras, behind = _handover_extras(world, rng)
    mine = [r for L in S_LENGTHS[::2] for r in _boundary_reads(world, L)][::3]
    step = len(mine) // len(extras)
    assert step >= 1
    reads, where = [], {}
    for i, r in enumerate(mine):          # interleaved, not grouped: one hand-over read after every `step` of the others
        reads.append(r)
        if i % step == step - 1 and i // step < len(extras):
            where[i // step] = len(reads)
            reads.append(extras[i // step])
    assert len(where) == len(extras)
    return reads, [where[i] for i in behind]


def test_handover_to_count_kernel_in_one_batch(world_s):
    """(b): reads the variants kernel answers and reads it marks for count_kernel, interleaved in one batch, under every
    policy -- what is handed over changes with the policy's seed length (under seed_len 32 the 29..32-nt reads are the
    variants kernel's own, L > 3 K)."""
    reads, behind = _handover_batch(world_s)
    lens = {len(r) for r in reads}
    assert lens >= {1, 2, 4, 7} | set(range(21, 33)) | set(S_LENGTHS[::2])
    wants = _check(world_s, reads)
    # some of the 29..32-nt reads align with their one mismatch behind base 28 (count_kernel's: L > seed_len)
    assert len(behind) >= 8 and all(len(reads[i]) >= 29 for i in behind)
    assert sum(wants[(28, 1, 2)][i][0] == 1 for i in behind) >= 8
    assert all(w == (255, 0) for r, w in zip(reads, wants[(28, 1, 2)]) if len(r) == 1)    # L <= max_mm_seed
    assert any(w[1] == 255 for r, w in zip(reads, wants[(28, 1, 2)]) if len(r) == 2)


@pytest.mark.parametrize("which", ["S", "M"])
def test_variants_kernel_alone_answers_every_read_that_fits(world_s, world_m, which):
    """`count_variants` = 2 (no count_kernel behind it): a read with 8 <= K <= L <= min(seed_len, 32) comes back answered,
    and right; every other read of more than one base comes back marked 254.  This is what notices a kernel that picks
    too small a table and quietly leaves its reads to count_kernel -- same answers, twelve times slower."""
    world = world_s if which == "S" else world_m
    if which == "S":
        reads, _ = _handover_batch(world)
    else:
        reads = [r for L in (10, 11, 16, 20, 22) for r in _boundary_reads(world, L)[:40]]
        reads += [r[:L] for L in (4, 8, 9) for r in _boundary_reads(world, 12)[:20]]      # K = 4, 6: not this kernel's
        reads += [world.seqs[0][100:100 + L] for L in (29, 32)] + ["G"]
    rs = _read_set(world.eng, reads)
    for policy in POLICIES:
        want = world.expect(reads, policy)
        got = _run(world, rs, policy, 2)
        n_fit = 0
        for r, g, w in zip(reads, got, want):
            L = len(r)
            if L <= policy[1]:
                assert g == (255, 0), (r, policy, g)
            elif world.table_k(L) >= 8 and L <= min(policy[0], 32):
                assert g == w, (r, policy, "got", g, "scan", w)
                n_fit += 1
            else:
                assert g[0] == TODO, (r, policy, g)
        assert n_fit >= 100
        assert sum(1 for r in reads if len(r) > 1 and not (world.table_k(len(r)) >= 8 and len(r) <= min(policy[0], 32))) >= 10


def test_entry_ends_short_entries_and_the_library_n(world_s):
    """(c): first and last L bases of entries, reads hanging one base over an entry's end (they must not align there: the
    text holds the next entry's first base right behind), a read equal to a whole 17-base entry, reads longer than it,
    the last bases of the text, both sides of the library N and reads across it."""
    w, seqs = world_s, world_s.seqs
    assert len(seqs[2]) == 17 and seqs[4][60] == "N"
    reads, over = [], []
    for L in (9, 12, 17, 18, 20, 27):
        for e in (0, 1, 3, 4, len(seqs) - 1):
            reads += [seqs[e][:L], seqs[e][-L:]]
            nxt = seqs[e + 1][0] if e + 1 < len(seqs) else "A"
            over.append(len(reads))
            reads.append(seqs[e][-(L - 1):] + nxt)            # one base over the end (of the text, for the last entry)
            over.append(len(reads))
            reads.append(seqs[e - 1][-1] + seqs[e][:L - 1] if e else "C" + seqs[e][:L - 1])   # one base in front of the start
        # the library N: up to it, from behind it, and across it with each base in its place
        reads += [seqs[4][60 - L:60], seqs[4][61:61 + L]]
        if L <= 27:
            reads += [seqs[4][60 - 5:60] + b + seqs[4][61:61 + L - 6] for b in "ACGT"]
    short = seqs[2]
    reads += [short, short + seqs[3][0], seqs[1][-1] + short, seqs[1][-2:] + short + seqs[3][:2], short[1:], short[:-1]]
    reads += [_sub(short, p, 0) for p in (0, 7, 8, 9, 16)]
    reads += [_sub(r, p, 1) for r in list(reads) if len(r) >= 9 for p in (0, len(r) // 2, len(r) - 1)]
    wants = _check(w, reads)
    want = wants[POLICIES[0]]
    assert want[reads.index(short)] == (0, 1) and want[reads.index(short + seqs[3][0])] == (255, 0)
    # what hangs over an end aligns nowhere (12 bases and more: chance hits elsewhere in 12 kb are out of reach)
    assert all(want[i] == (255, 0) for i in over if len(reads[i]) >= 12)
    assert all(want[reads.index(seqs[4][60 - 5:60] + b + seqs[4][61:61 + 14])] == (255, 0) for b in "ACGT")
    assert want[reads.index(seqs[-1][-20:])] == (0, 1) and want[reads.index(seqs[4][61:61 + 20])] == (0, 1)


def test_count_clamps_at_255(engine):
    """(d): a 24-mer written 300 times.  255 where the scan counts 255 or more -- the clamp, not a lookup cut short: no
    k-mer of the tables used has more than 4096 rows."""
    rng = np.random.default_rng(904)
    mer = _rnd(rng, 24)
    body = "".join(mer + _rnd(rng, 1) for _ in range(300))
    seqs = [_rnd(rng, 700) + body + _rnd(rng, 300), _rnd(rng, 900)]
    assert max(_max_kmer_rows(seqs, k) for k in (8, 9)) <= MAX_ROWS
    w = _World(engine, "S2", ["rep", "plain"], seqs)
    assert w.ks == [9, 8, 6, 4]
    r20 = mer[:20]
    reads = [r20, _sub(r20, 10, 0), mer[6:18], mer, seqs[1][100:120]]
    reads += [_sub(r20, p, k) for p in (8, 9, 10, 11, 0, 19) for k in range(3)]      # K = 9: L-K-1 .. K and the ends
    reads += [_sub(mer[6:18], p, 1) for p in range(12)]
    want = _check(w, reads)[POLICIES[0]]
    assert sum(w.scan_count(r, POLICIES[0]) >= 255 for r in reads[:3]) >= 2
    assert want[0] == (0, 255) and want[1] == (1, 255) and want[2] == (0, 255) and want[4] == (0, 1)


def test_grid_stride_above_65536_reads(world_s):
    """(e): the whole case set of (a) on S tiled to 70 001 reads under a seeded permutation -- more half-waves than the
    variants kernel's largest grid (n_cu * 32 * 8 = 65 536 on 256 CUs), not a multiple of 8; one ReadSet for both
    kernels, the expected values indexed out of the per-case answers."""
    from mirge_amd.engine import ReadSet
    cases = [r for L in S_LENGTHS for r in _boundary_reads(world_s, L)]
    want = np.array(world_s.expect(cases, POLICIES[0]), dtype=np.int64)
    idx = np.random.default_rng(905).permutation(np.resize(np.arange(len(cases)), 70001))
    small = _read_set(world_s.eng, cases)
    words, lens = small.words.cpu().numpy().view(np.uint64)[:, idx], small.lens.cpu().numpy()[idx]
    rs = ReadSet(np.ascontiguousarray(words), np.ascontiguousarray(lens), None, None, device=world_s.eng.device)
    assert rs.W == 1 and rs.n == 70001 and rs.nmask is None
    for variants in (1, 0, 2):
        got = np.array(_run(world_s, rs, POLICIES[0], variants), dtype=np.int64)
        bad = np.flatnonzero((got != want[idx]).any(axis=1))
        assert bad.size == 0, (variants, bad.size, [(cases[idx[i]], got[i].tolist(), want[idx[i]].tolist()) for i in bad[:5]])


def test_saturated_lookup_says_undecided_not_unaligned(engine):
    """A K-mer with more than 4096 rows: both kernels walk its first 4096 rows only.  The header's contract is
    count == 255 ("too repetitive to be walked"), ALSO when none of the walked rows aligned: (255, 255) = undecided, which
    a2i.EngineGenome turns into "not unique" (tests/test_a2i.py).  Here A x 6000 and, elsewhere, ONE occurrence of
    A x 9 + TTGCATGCA (18 nt = 2 K: no variants): lookup A (A x 9) is cut short before it reaches the occurrence, and B's
    exact hit is not B's to count -- before the fix both kernels answered (255, 0), "does not align"."""
    rng = np.random.default_rng(906)
    hit = "A" * 9 + "TTGCATGCA"
    seqs = ["A" * 6000, _rnd(rng, 200) + "C" + hit + "C" + _rnd(rng, 200)]
    w = _World(engine, "sat", ["polyA", "other"], seqs)
    assert w.ks == [9, 8, 6, 4] and w.table_k(18) == 9
    # on the CPU: the occurrence lies beyond row 4096 of the A x 9 interval of the suffix array
    text = "".join(seqs)
    at = text.index(hit)
    assert text.count(hit) == 1 and at == 6201
    pos = (w.ix.view()["sa"] & np.uint64(0xFFFFFFFF)).astype(np.int64)
    starts = np.array([p for p in range(len(text) - 8) if text[p:p + 9] == "A" * 9], dtype=np.int64)
    rows = np.flatnonzero(np.isin(pos, starts))
    assert rows.size == starts.size > MAX_ROWS and rows[-1] - rows[0] + 1 == rows.size      # one interval
    assert int(np.flatnonzero(pos == at)[0]) - int(rows[0]) >= MAX_ROWS
    reads = ["A" * 20, "A" * 10 + "C" + "A" * 9, hit]
    rs = _read_set(engine, reads)
    for policy in ((28, 1, 2), (28, 1, 1)):
        scan = [model.best_stratum(w.olib, r, *policy) for r in reads]
        assert scan[0][0] == 0 and scan[0][1] >= 255 and scan[1][0] == 1 and scan[1][1] >= 255 and scan[2] == (0, 1)
        for variants in (1, 0):
            got = _run(w, rs, policy, variants)
            assert got[0] == (0, 255) and got[1] == (1, 255), (policy, variants, got)
            assert got[2][1] == 255 and got[2][0] in (0, 255), (policy, variants, got)
