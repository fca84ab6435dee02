"""The edit sweep: libraries and reads that walk the grid (read length x mismatch position x distance to the
entry's ends) on which the alignment kernels take their position-dependent shortcuts -- pigeonhole seeds of
floor(R / (V + 1)) bases, the stored context of a wide row, the six- and eight-bit segment-room fields of a
row, the 5-base anchors of the pair tables, the four anchors of the 2-mismatch pass, the seed boundary at base
28, the `-5 1 -3 2` trims.  Plain numpy, no GPU, deterministic from a seed.

Every case carries its provenance (entry, offset, L, edit positions, site class); `in_policy` says from that
alone whether the planted alignment satisfies a policy.  What a read's answer IS comes from the exhaustive
scan (oracle.model.align_batch): a read may also hit elsewhere by chance, and then the scan's answer is the
expected one (tests/test_edit_sweep_cpu.py bounds how often that happens)."""
import collections
import itertools

import numpy as np

LENGTHS = tuple(range(16, 33))
# (seed_len, max_mm_seed, max_mm_total, trim5, trim3): the five policies of engine.MIRGE_PASS_TABLE
POLICIES = ((28, 0, 2, 0, 0), (1024, 0, 0, 0, 0), (28, 1, 2, 0, 0), (1024, 1, 1, 0, 0), (1024, 2, 2, 1, 2))
EXACT_POLICIES = (POLICIES[0], POLICIES[1])
ONE_MM_POLICIES = (POLICIES[2], POLICIES[3])
TWO_MM_POLICY = POLICIES[4]
# the large library does not see the last one: a trimmed 13-mer within two mismatches occurs a dozen times by
# chance in 1.2 Mbases
LARGE_POLICIES = POLICIES[:4]
XLARGE_POLICIES = ONE_MM_POLICIES

PAIR_LENGTHS_LARGE = (16, 19, 20, 22, 23, 24, 28, 29, 32)   # seed regions at both ends of every piece / anchor layout
# (the scan costs 3.5 x the large library's: an anchor-pair length, the bucket lengths, one beyond the seed; no 16-nt pairs,
# whose 16 bases within one mismatch occur by chance in 4.2 Mbases for one read in twenty)
PAIR_LENGTHS_XLARGE = (19, 22, 23, 29)
TRIPLE_LENGTHS = (16, 19, 22, 28, 32)
SITE_CLASSES = ("start", "start+1", "end", "end-1", "whole", "lib_first", "lib_last", "off63", "off255", "off300")
N_SITE_CLASSES = ("n1_before", "n1_after", "n5_before", "n5_after")
PAIR_SITE = "off300"          # where the two- and three-substitution reads are cut

Case = collections.namedtuple("Case", "read entry offset L edits site")
Sweep = collections.namedtuple("Sweep", "name names seqs cases")


def _rand_seq(rng, n):
    return np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, int(n))].tobytes().decode("ascii")


def substitute(s, edits, rots=None):
    """`s` with the base at every position j of `edits` rotated by 1 + j % 3 (or 1 + rots[i]): never the base it had."""
    r = list(s)
    for i, j in enumerate(edits):
        r[j] = "ACGT"[("ACGT".index(r[j]) + 1 + (j if rots is None else rots[i]) % 3) & 3]
    return "".join(r)


def in_policy(L, edits, policy):
    """(does the planted alignment satisfy the policy, with how many mismatches) from the provenance alone: the
    edits inside the trimmed read, those inside its first min(L', seed_len) bases against max_mm_seed, all of
    them against max_mm_total."""
    seed_len, mm_seed, mm_total, t5, t3 = policy
    Lt = L - t5 - t3
    inside = [j - t5 for j in edits if t5 <= j < L - t3]
    if Lt <= mm_seed:          # (a read not longer than the allowed seed mismatches is skipped)
        return False, len(inside)
    seed = min(Lt, seed_len)
    ok = sum(1 for j in inside if j < seed) <= mm_seed and len(inside) <= mm_total
    return ok, len(inside)


def trimmed(read, policy):
    t5, t3 = policy[3], policy[4]
    return read[t5:len(read) - t3]


class _Layout:
    """Entries of one library and the sites (entry, offset) of every (site class, L)."""

    def __init__(self, rng, big_len, n_mid, n_hosts):
        # one long first and last entry, the whole-read entries, `n_mid` entries of 60..140 nt (the first 5 x 17 of
        # them at least 100 nt: they carry the start / end / offset-63 sites), the big entries, the N hosts
        t = len(LENGTHS)
        kinds = [("whole", L) for L in LENGTHS]
        kinds += [("mid", int(rng.integers(100, 141)) if i < 5 * t else int(rng.integers(60, 141))) for i in range(n_mid)]
        kinds += [("big", n) for n in big_len] + [("host", 400)] * n_hosts
        order = rng.permutation(len(kinds))
        kinds = [("first", 130)] + [kinds[i] for i in order] + [("last", 130)]
        self.seqs = [_rand_seq(rng, n) for _, n in kinds]
        self.names = ["%s%d" % (k, i) for i, (k, _) in enumerate(kinds)]
        self.by_kind = collections.defaultdict(list)
        for i, (k, _) in enumerate(kinds):
            self.by_kind[k].append(i)
        self.rng = rng

    def sites(self, L):
        t = L - LENGTHS[0]
        mid, big, T = self.by_kind["mid"], self.by_kind["big"], len(LENGTHS)
        # (`mid` is in library order; which of them are the long ones does not matter as long as each site fits)
        long_mid = [e for e in mid if len(self.seqs[e]) >= 100]
        pick = lambda k: long_mid[k * T + t]
        n = lambda e: len(self.seqs[e])
        whole = self.by_kind["whole"][[len(self.seqs[e]) for e in self.by_kind["whole"]].index(L)]
        b255, b300 = big[t % len(big)], big[(t + 1) % len(big)]
        off300 = 300 + 2 * t if n(b300) <= 400 else int(self.rng.integers(300, n(b300) - 400))
        out = {"start": (pick(0), 0), "start+1": (pick(1), 1), "end": (pick(2), n(pick(2)) - L),
               "end-1": (pick(3), n(pick(3)) - L - 1), "whole": (whole, 0), "lib_first": (0, 0),
               "lib_last": (len(self.seqs) - 1, n(len(self.seqs) - 1) - L), "off63": (pick(4), 63 + (t & 1)),
               "off255": (b255, 255 + (t & 1)), "off300": (b300, off300)}
        if n(big[0]) > 400 and (t & 1):
            # a large library: every other length takes the ends of the long entries instead (segment room far beyond
            # what a row's fields hold on one side, none on the other)
            out["start"], out["start+1"] = (big[1], 0), (big[1], 1)
            out["end"], out["end-1"] = (big[1], n(big[1]) - L), (big[1], n(big[1]) - L - 1)
        return out


def _cases_of(layout, pair_lengths, triple_lengths):
    cases = []

    def add(site, e, o, L, edits):
        cases.append(Case(substitute(layout.seqs[e][o:o + L], edits), e, o, L, tuple(edits), site))
    for L in LENGTHS:
        sites = layout.sites(L)
        for site in SITE_CLASSES:
            e, o = sites[site]
            assert 0 <= o and o + L <= len(layout.seqs[e]), (site, L)
            add(site, e, o, L, ())
            for j in range(L):
                add(site, e, o, L, (j,))
        e, o = sites[PAIR_SITE]
        if L in pair_lengths:
            for j1, j2 in itertools.combinations(range(L), 2):
                add(PAIR_SITE, e, o, L, (j1, j2))
        if L in triple_lengths:
            mid = L // 2
            for j1, j2 in itertools.combinations([j for j in range(L) if j != mid], 2):
                add(PAIR_SITE, e, o, L, tuple(sorted((j1, j2, mid))))
    return cases


def _unique_triples(layout, cases, policy=TWO_MM_POLICY, max_len=18):
    """A three-substitution read of at most `max_len` nt whose three edits lie inside the trimmed read is what the
    2-mismatch policy must REJECT -- but 13..15 trimmed bases within two mismatches occur by chance in 30 kbases
    for a third of such reads.  Those reads get the first rotation of their substituted bases that leaves no
    window of the library within two mismatches of the trimmed read (a condition on the input, checked here with
    numpy alone)."""
    text = np.frombuffer("#".join(layout.seqs).encode("ascii"), dtype=np.uint8)
    out = []
    for c in cases:
        ok, _ = in_policy(c.L, c.edits, policy)
        if len(c.edits) != 3 or c.L > max_len or ok:
            out.append(c)
            continue
        src = layout.seqs[c.entry][c.offset:c.offset + c.L]
        for rots in itertools.product(range(3), repeat=3):
            r = substitute(src, c.edits, rots)
            t = np.frombuffer(trimmed(r, policy).encode("ascii"), dtype=np.uint8)
            win = np.lib.stride_tricks.sliding_window_view(text, len(t))
            if int((win != t).sum(axis=1).min()) > policy[2]:
                break
        else:
            raise AssertionError("no rotation of %r is free of chance hits" % (c,))
        out.append(c._replace(read=r))
    return out


def _finish(name, names, seqs, cases, seed):
    reads = [c.read for c in cases]
    assert len(set(reads)) == len(reads), "%s: the sweep's reads are not distinct" % name
    assert all(set(r) <= set("ACGT") and 16 <= len(r) <= 32 for r in reads)
    order = np.random.default_rng(seed).permutation(len(cases))   # a tile holds mixed lengths
    return Sweep(name, list(names), list(seqs), [cases[i] for i in order])


def small_sweeps(seed=20240):
    """(small, small_n): about 35 kbases, below every large-library threshold; small_n is the same library with an N
    run of 1 and one of 5 planted inside its four host entries (segments != entries: the seg_ref / seg_off route),
    and the reads that end on the base before each run / start on the base after it on top of small's."""
    rng = np.random.default_rng(seed)
    lay = _Layout(rng, big_len=[400] * 8, n_mid=280, n_hosts=4)
    cases = _unique_triples(lay, _cases_of(lay, LENGTHS, TRIPLE_LENGTHS))
    small = _finish("small", lay.names, lay.seqs, cases, seed + 1)
    seqs_n = list(lay.seqs)
    hosts = lay.by_kind["host"]
    for h in hosts:
        s = seqs_n[h]
        seqs_n[h] = s[:150] + "N" + s[151:250] + "NNNNN" + s[255:]
    n_cases = []
    for L in LENGTHS:
        h = hosts[(L - LENGTHS[0]) % len(hosts)]
        for site, o in (("n1_before", 150 - L), ("n1_after", 151), ("n5_before", 250 - L), ("n5_after", 255)):
            src = seqs_n[h][o:o + L]
            assert "N" not in src and (seqs_n[h][o - 1] == "N" or seqs_n[h][o + L] == "N")
            for edits in [()] + [(j,) for j in range(L)]:
                n_cases.append(Case(substitute(src, edits), h, o, L, edits, site))
    small_n = _finish("small_n", lay.names, seqs_n, cases + n_cases, seed + 2)
    return small, small_n


def large_sweep(seed=20241):
    """large: three entries of 400 kbases and 200 short ones, 1.2 Mbases (between 2^20 and 2^22): device-built jump
    tables, wide rows, seed buckets, the device-built pair tables.  (A seed launch searches a library of at most 2^22
    bases through an index rebuilt from its entries, without buckets: xlarge_sweep.)"""
    rng = np.random.default_rng(seed)
    lay = _Layout(rng, big_len=[400_000] * 3, n_mid=183, n_hosts=0)
    n_bases = sum(len(s) for s in lay.seqs)
    assert (1 << 20) <= n_bases <= (1 << 22)
    return _finish("large", lay.names, lay.seqs, _cases_of(lay, PAIR_LENGTHS_LARGE, ()), seed + 1)


def xlarge_sweep(seed=20242):
    """xlarge: the same shape just past 2^22 bases (three entries of 1.4 Mbases), the size from which a seed launch
    searches the library's own arrays -- seed buckets, position lists, wide rows -- in wave_seed_kernel.  For the two
    one-mismatch policies only (XLARGE_POLICIES)."""
    rng = np.random.default_rng(seed)
    lay = _Layout(rng, big_len=[1_400_000] * 3, n_mid=183, n_hosts=0)
    assert sum(len(s) for s in lay.seqs) > (1 << 22)
    return _finish("xlarge", lay.names, lay.seqs, _cases_of(lay, PAIR_LENGTHS_XLARGE, ()), seed + 1)


def coverage(cases):
    """{(site, L): set of edit tuples}."""
    cov = collections.defaultdict(set)
    for c in cases:
        cov[(c.site, c.L)].add(c.edits)
    return cov


# ---- comparing an aligner's answers with the scan's, and saying where in the grid they differ ----
_SCANS = {}


def scan_answers(sweep, policy):
    """The exhaustive scan on the trimmed reads: an int32 array (n, 3) of (entry, offset, mismatches), -1 = unaligned.
    Computed once per (library, policy) and shared by every test of a session; read-only."""
    key = (sweep.name, len(sweep.cases), tuple(policy))
    if key not in _SCANS:
        from oracle import model
        lib = model.Library(sweep.names, sweep.seqs)
        a = np.stack(model.align_batch(lib, [trimmed(c.read, policy) for c in sweep.cases], policy[0], policy[1], policy[2]), axis=1)
        a.setflags(write=False)
        _SCANS[key] = a
    return _SCANS[key]


def pass_dict(policy, lib=0):
    seed_len, mm_seed, mm_total, t5, t3 = policy
    return dict(lib=lib, seed_len=seed_len, max_mm_seed=mm_seed, max_mm_total=mm_total, trim5=t5, trim3=t3, min_len=0, max_len=255,
                poly_t=0)


def claimed(pass_id, ref_id, pos, mm, k):
    """(n, 3) array of what pass k claimed: (entry, offset, mismatches), -1 where it claimed nothing."""
    got = np.stack([np.asarray(ref_id, dtype=np.int32), np.asarray(pos, dtype=np.int32), np.asarray(mm).astype(np.int32)], axis=1)
    got[np.asarray(pass_id) != k] = -1
    return got


def grid_report(where, policy, cases, got, want, limit=10):
    """'' when the (n, 3) arrays agree; else the route and policy, the first `limit` failing cases with (L, site class,
    edit positions, got, want) and the failures counted by (L, first edit position)."""
    got, want = np.asarray(got).reshape(len(cases), 3), np.asarray(want).reshape(len(cases), 3)
    bad = np.flatnonzero((got != want).any(axis=1))
    if not len(bad):
        return ""
    lines = ["%s, policy %s: %d of %d reads differ from the scan" % (where, policy, len(bad), len(cases))]
    for i in bad[:limit]:
        c = cases[i]
        lines.append("  L=%d site=%s edits=%s got=%s want=%s" % (c.L, c.site, c.edits, tuple(int(x) for x in got[i]),
                                                                 tuple(int(x) for x in want[i])))
    cells = collections.Counter((cases[i].L, cases[i].edits[0] if cases[i].edits else None) for i in bad)
    ordered = sorted(cells.items(), key=lambda kv: (kv[0][0], -1 if kv[0][1] is None else kv[0][1]))
    lines.append("  by (L, first edit): " + ", ".join("%s: %d" % (k, v) for k, v in ordered))
    return "\n".join(lines)
