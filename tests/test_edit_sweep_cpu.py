"""The edit sweep (tests/edit_sweep.py) without a GPU: the grid is complete, the exhaustive scan is a usable
yardstick on it (nearly every read is answered at its planted site or, when the policy rules the planted
alignment out, not at all), and the CPU port -- the yardstick of most GPU tests -- equals the scan on every
read of every (library, policy), with and without the anchor-pair searches the GPU reports."""
import itertools

import numpy as np
import pytest

from oracle import model
from mirge_amd.engine import DEFAULT_WSTOP, MIRGE_PASS_TABLE
from tests import edit_sweep as es


@pytest.fixture(scope="module")
def sweeps(oracle_lib):
    small, small_n = es.small_sweeps()
    return {"small": small, "small_n": small_n, "large": es.large_sweep(), "xlarge": es.xlarge_sweep()}


def policies_of(name):
    return {"large": es.LARGE_POLICIES, "xlarge": es.XLARGE_POLICIES}.get(name, es.POLICIES)


def test_the_policies_are_the_pass_tables():
    assert set(es.POLICIES) == {row[3:8] for row in MIRGE_PASS_TABLE}


def test_in_policy_by_hand():
    assert es.in_policy(22, (), (1024, 0, 0, 0, 0)) == (True, 0)
    assert es.in_policy(22, (5,), (1024, 0, 0, 0, 0)) == (False, 1)
    assert es.in_policy(29, (28,), (28, 0, 2, 0, 0)) == (True, 1)          # behind the seed
    assert es.in_policy(29, (27,), (28, 0, 2, 0, 0)) == (False, 1)
    assert es.in_policy(32, (3, 28, 31), (28, 1, 2, 0, 0)) == (False, 3)   # the seed is fine, the total is not
    assert es.in_policy(32, (3, 4), (28, 1, 2, 0, 0)) == (False, 2)
    assert es.in_policy(22, (0, 5, 9, 21), (1024, 2, 2, 1, 2)) == (True, 2)   # two of the four edits are trimmed away
    assert es.in_policy(22, (0, 5, 9, 19), (1024, 2, 2, 1, 2)) == (False, 3)
    assert es.in_policy(22, (20,), (1024, 2, 2, 1, 2)) == (True, 0)


def test_grid_coverage(sweeps):
    """Every (L, j) at every site class, every pair / triple for the stated L: a later edit to the generator cannot thin
    the grid out silently."""
    for name, sw in sweeps.items():
        cov = es.coverage(sw.cases)
        classes = es.SITE_CLASSES + (es.N_SITE_CLASSES if name == "small_n" else ())
        assert {k[0] for k in cov} == set(classes), name
        for site, L in itertools.product(classes, es.LENGTHS):
            assert {()} | {(j,) for j in range(L)} <= cov[(site, L)], (name, site, L)
        pair_lengths = {"large": es.PAIR_LENGTHS_LARGE, "xlarge": es.PAIR_LENGTHS_XLARGE}.get(name, es.LENGTHS)
        assert name == "xlarge" or {16, 19, 20, 22, 23, 24, 28, 29, 32} <= set(pair_lengths)
        for L in pair_lengths:
            assert set(itertools.combinations(range(L), 2)) <= cov[(es.PAIR_SITE, L)], (name, L)
        if name in ("small", "small_n"):
            assert {16, 19, 22, 28, 32} <= set(es.TRIPLE_LENGTHS)
            for L in es.TRIPLE_LENGTHS:
                want = {tuple(sorted((a, b, L // 2))) for a, b in itertools.combinations([j for j in range(L) if j != L // 2], 2)}
                assert want <= cov[(es.PAIR_SITE, L)], (name, L)
        reads = [c.read for c in sw.cases]
        assert len(set(reads)) == len(reads) and all("N" not in r and 16 <= len(r) <= 32 for r in reads)
        # provenance: the read is the entry's bases with exactly its edit positions changed
        for c in sw.cases:
            src = sw.seqs[c.entry][c.offset:c.offset + c.L]
            assert len(src) == c.L == len(c.read) and tuple(j for j in range(c.L) if src[j] != c.read[j]) == c.edits
        # a tile of 256 reads holds mixed lengths
        lens = np.array([c.L for c in sw.cases])
        assert all(len(set(lens[i:i + 256])) >= 12 for i in range(0, len(lens) - 255, 256)), name


def test_site_classes_are_where_they_say(sweeps):
    for name, sw in sweeps.items():
        n_entries = len(sw.seqs)
        for c in sw.cases:
            n = len(sw.seqs[c.entry])
            room = n - c.offset - c.L
            s = sw.seqs[c.entry]
            end = c.offset + c.L
            ok = {"start": lambda: c.offset == 0, "start+1": lambda: c.offset == 1, "end": lambda: room == 0, "end-1": lambda: room == 1,
                  "whole": lambda: c.offset == 0 and room == 0, "lib_first": lambda: c.entry == 0 and c.offset == 0,
                  "lib_last": lambda: c.entry == n_entries - 1 and room == 0, "off63": lambda: c.offset in (63, 64) and room > 0,
                  "off255": lambda: c.offset in (255, 256) and room > 0, "off300": lambda: c.offset >= 300 and room > 0,
                  "n1_before": lambda: s[end] == "N" and s[end + 1] != "N", "n1_after": lambda: s[c.offset - 1] == "N" and s[c.offset - 2] != "N",
                  "n5_before": lambda: s[end:end + 5] == "NNNNN", "n5_after": lambda: s[c.offset - 5:c.offset] == "NNNNN"}[c.site]()
            assert ok, (name, c)
        if name == "small_n":
            assert sum(s.count("N") for s in sw.seqs) == 4 * 6 and sw.names == sweeps["small"].names
        else:
            assert not any("N" in s for s in sw.seqs)
        n_bases = sum(len(s) for s in sw.seqs)
        lo, hi = {"large": (1 << 20, 1 << 22), "xlarge": ((1 << 22) + 1, 5 << 20)}.get(name, (25_000, 40_000))
        assert lo <= n_bases <= hi, (name, n_bases)


@pytest.mark.parametrize("name", ["small", "small_n", "large", "xlarge"])
def test_the_scan_is_the_yardstick(sweeps, name):
    """A condition on the INPUTS: at least 99 % of the in-policy reads come back at the planted (entry, offset + trim5)
    with the planted mismatch count, at least 99 % of the out-of-policy reads unaligned.  The rest are chance hits and
    ties, for which the scan's answer is the expected one.  (A seed that gives less: change the seed or the library.)"""
    sw = sweeps[name]
    for policy in policies_of(name):
        scan = es.scan_answers(sw, policy)
        verdict = [es.in_policy(c.L, c.edits, policy) for c in sw.cases]
        inside = np.array([ok for ok, _ in verdict])
        planted = np.array([(c.entry, c.offset + policy[3], k) for c, (_, k) in zip(sw.cases, verdict)], dtype=np.int32)
        at_site = (scan == planted).all(axis=1)
        unaligned = (scan == -1).all(axis=1)
        assert inside.sum() > 100 and (~inside).sum() > (0 if policy[1] == 2 else 100), (name, policy)
        f_in, f_out = at_site[inside].mean(), unaligned[~inside].mean()
        print("%s %s: %d reads, in-policy at the planted site %.4f (%d), out-of-policy unaligned %.4f (%d)" %
              (name, policy, len(sw.cases), f_in, inside.sum(), f_out, (~inside).sum()))
        assert f_in >= 0.99 and f_out >= 0.99, (name, policy, f_in, f_out)
        # a read the scan answers somewhere else is a hit at least as good, never a worse one
        moved = inside & ~at_site
        assert (scan[moved, 2] <= planted[moved, 2]).all() and (scan[moved, 2] >= 0).all(), (name, policy)


@pytest.fixture(scope="module")
def indexes(native_lib, sweeps):
    from mirge_amd.index import FmIndex
    return {name: FmIndex.build(sw.names, sw.seqs) for name, sw in sweeps.items()}


@pytest.mark.parametrize("name", ["small", "small_n", "large", "xlarge"])
def test_the_port_equals_the_scan(sweeps, indexes, name):
    """model.fm_cascade (ftab, the default wstop; also with `pair_anchor` as the GPU reports it: 4 for the 2-mismatch
    policy, 5 for the one-mismatch policies on the large library) as a single-pass cascade against the scan: pass id,
    entry, offset, mismatches of every read, and the processed / aligned counters."""
    from mirge_amd import pack
    sw = sweeps[name]
    view = indexes[name].view()
    words, lens, nmask = pack.pack_reads([c.read for c in sw.cases])
    assert words.shape[0] == 1 and nmask is None
    for policy in policies_of(name):
        scan = es.scan_answers(sw, policy)
        anchors = (0, 4) if policy[1] == 2 else (0, 5) if (policy[1] == 1 and name in ("large", "xlarge")) else (0,)
        for pair_anchor in anchors:
            p = dict(es.pass_dict(policy), pair_anchor=pair_anchor)
            ref = model.fm_cascade([view], [p], words, lens, None, wstop=DEFAULT_WSTOP, ftab=True)
            got = es.claimed(ref["pass_id"], ref["ref_id"], ref["pos"], ref["mm"], 0)
            report = es.grid_report("CPU port (pair_anchor %d) on %s" % (pair_anchor, name), policy, sw.cases, got, scan)
            assert not report, report
            assert set(np.unique(ref["pass_id"]).tolist()) <= {0, -1}
            assert (int(ref["stats"][0][0]), int(ref["stats"][0][1])) == (len(sw.cases), int((scan[:, 0] >= 0).sum())), (name, policy)
