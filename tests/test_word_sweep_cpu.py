"""The word sweep (tests/word_sweep.py) without a GPU: the grid is complete and every read is what its provenance says,
each batch packs into the stated number of words with an N mask, the exhaustive scan is a usable yardstick on it (the
bars of tests/test_edit_sweep_cpu.py), and the CPU port equals the scan on every read of every (batch, policy) -- with
the N masks, with and without the anchor pairs of the 2-mismatch policy, and on the poly-T class under `poly_t` = 1."""
import itertools

import numpy as np
import pytest

from oracle import model
from mirge_amd.engine import DEFAULT_WSTOP
from tests import edit_sweep as es
from tests import word_sweep as ws

WORDS = (2, 4, 8)


@pytest.fixture(scope="module")
def sweeps(oracle_lib):
    return ws.word_sweeps()


def test_the_lengths_are_the_edges_of_every_word_count():
    from mirge_amd import pack
    for W, lengths in ws.WORD_LENGTHS.items():
        assert {pack.words_for(L) for L in lengths} == {W}
        assert {16 * W + 1, 32 * W - 1, min(32 * W, 255)} <= set(lengths)   # the first, the last but one, the last length of W words
    assert ws.boundary_positions(16) == (0, 1, 12, 13, 14, 15)
    assert ws.boundary_positions(64) == (0, 1, 26, 27, 28, 29, 31, 32, 33, 60, 61, 62, 63)
    assert ws.boundary_positions(129) == (0, 1, 26, 27, 28, 29, 31, 32, 33, 63, 64, 65, 95, 96, 97, 125, 126, 127, 128)
    assert set(range(31, 255, 32)) | set(range(32, 255, 32)) | set(range(33, 255, 32)) <= set(ws.boundary_positions(255))


def test_poly_t_view_by_hand():
    body = "ACGTACGTACG"
    assert ws.poly_t_view(body + "TTT") == body
    assert ws.poly_t_view(body + "TT") is None                      # fewer than three T
    assert ws.poly_t_view(body[:10] + "TTT") is None                # fewer than 11 bases left
    assert ws.poly_t_view(body + "TTNTTT") == body + "TTN"          # an N is no T
    assert ws.poly_t_view(body + "TTTTNTT") is None


@pytest.mark.parametrize("W", WORDS)
def test_grid_coverage(sweeps, W):
    """Every (site, L, j) with a substitution and with an N, every pair of B(L) in its four kinds and with the third
    edit at L // 2, each read its source with exactly its edits, the batch W words wide with an N mask: a later edit to
    the generator cannot thin the grid out silently."""
    sw = sweeps["w%d" % W]
    cov = ws.coverage(sw.cases)
    assert {k[0] for k in cov} == set(ws.SITE_CLASSES + ws.N_SITE_CLASSES)
    assert {k[1] for k in cov} == set(ws.SHORT_LENGTHS + ws.WORD_LENGTHS[W])
    for site, L in itertools.product(ws.SITE_CLASSES + ws.N_SITE_CLASSES, ws.lengths_of(W)):
        want = {()} | {((j, k),) for j in range(L) for k in "SN"}
        assert want <= cov[(site, L)], (W, site, L)
    for L in ws.lengths_of(W):
        B = ws.boundary_positions(L)
        assert {0, 1, 26 if L > 26 else 0, L - 4, L - 1} <= set(B) and all(m in B for m in range(32, L, 32)), L
        for j1, j2 in itertools.combinations(B, 2):
            for k1, k2 in itertools.product("SN", repeat=2):
                assert ((j1, k1), (j2, k2)) in cov[(ws.PAIR_SITE, L)], (W, L, j1, j2)
                if L // 2 not in (j1, j2):
                    assert tuple(sorted(((j1, k1), (j2, k2), (L // 2, "S")))) in cov[(ws.PAIR_SITE, L)], (W, L, j1, j2)
    reads = [c.read for c in sw.cases]
    assert len(set(reads)) == len(reads)
    for c in sw.cases:   # provenance
        src = sw.seqs[c.entry][c.offset:c.offset + c.L]
        assert len(src) == c.L == len(c.read) and "N" not in src
        assert tuple(j for j in range(c.L) if src[j] != c.read[j]) == c.edits, c
    words, lens, nmask = ws.pack(sw)
    assert words.shape == (W, len(sw.cases)) and nmask is not None and nmask.shape == words.shape
    assert [int(x) for x in lens] == [c.L for c in sw.cases]
    n_words = (lens.astype(np.int64) + 31) // 32
    for k in range(W):      # a short read's upper words are zero, a long read's N sits in the word of its position
        assert not words[k, n_words <= k].any() and not nmask[k, n_words <= k].any()
        assert nmask[k].any()
    # a tile of 256 reads holds mixed lengths
    assert all(len(set(lens[i:i + 256].tolist())) >= 6 for i in range(0, len(lens) - 255, 256))


def test_site_classes_are_where_they_say(sweeps):
    sw = sweeps["w8"]
    n_bases = sum(len(s) for s in sw.seqs)
    assert 35_000 <= n_bases <= 60_000, n_bases
    assert sum(s.count("N") for s in sw.seqs) == 4 * 6
    assert len(sw.seqs[0]) >= 600 and len(sw.seqs[-1]) >= 600
    assert all(sweeps[k].seqs == sw.seqs and sweeps[k].names == sw.names for k in sweeps)
    for W in WORDS:
        for c in sweeps["w%d" % W].cases:
            s = sweeps["w%d" % W].seqs[c.entry]
            room, end = len(s) - c.offset - c.L, c.offset + c.L
            ok = {"start": lambda: c.offset == 0 and 300 <= len(s) <= 700, "end": lambda: room == 0 and 300 <= len(s) <= 700,
                  "whole": lambda: c.offset == 0 and room == 0, "lib_first": lambda: c.entry == 0 and c.offset == 0,
                  "lib_last": lambda: c.entry == len(sw.seqs) - 1 and room == 0,
                  "mid": lambda: c.offset >= 300 and room > 0 and len(s) <= 700,
                  "n1_before": lambda: s[end] == "N" and s[end + 1] != "N", "n1_after": lambda: s[c.offset - 1] == "N" and s[c.offset - 2] != "N",
                  "n5_before": lambda: s[end:end + 5] == "NNNNN", "n5_after": lambda: s[c.offset - 5:c.offset] == "NNNNN"}[c.site]()
            assert ok, (W, c)


@pytest.mark.parametrize("W", WORDS)
def test_poly_t_class(sweeps, W):
    """Runs of 2, 3, 4 and 9 that begin at b - 1, b and b + 1 for every boundary b of the batch, half of them with an N
    inside, behind an entry's bases cut at its start, its end and its middle."""
    sw = sweeps["w%d_polyt" % W]
    seen = set()
    for c in sw.cases:
        place, rest = c.site.split(":")
        with_n = rest.endswith("n")
        run, start = (int(x) for x in rest.rstrip("n")[1:].split("@"))
        assert c.L == start + run == len(c.read)
        assert c.read[start:].replace("N", "T") == "T" * run and c.read[start - 1] != "T" and (c.read.count("N") == 1) == with_n
        s = sw.seqs[c.entry]
        src = s[c.offset:c.offset + start] + "T" * run
        assert tuple(j for j in range(c.L) if src[j] != c.read[j]) == tuple(sorted(c.edits)), c
        assert {"start": c.offset == 0, "end": c.offset + start == len(s), "mid": c.offset >= 300 and c.offset + start < len(s)}[place]
        seen.add((place, run, start, with_n))
    want = {(p, r, b + d, n) for p in ("start", "end", "mid") for r in ws.TAILS for b in ws.TAIL_BOUNDS[W] for d in (-1, 0, 1) for n in (False, True)}
    assert seen == want and 32 * W // 2 in ws.TAIL_BOUNDS[W]
    words, lens, nmask = ws.pack(sw)
    assert words.shape[0] == W and nmask is not None
    took = [ws.poly_t_view(c.read) for c in sw.cases]
    assert sum(v is None for v in took) > 50 and sum(v is not None and "N" in v for v in took) > 20


@pytest.mark.parametrize("W", WORDS)
def test_the_scan_is_the_yardstick(sweeps, W):
    """The condition on the INPUTS of tests/test_edit_sweep_cpu.py, with its bars: at least 99 % of the in-policy reads
    come back at the planted (entry, offset + trim5) with the planted mismatch count, at least 99 % of the out-of-policy
    reads unaligned; a read that moved is a hit at least as good."""
    sw = sweeps["w%d" % W]
    for policy in es.POLICIES:
        scan = es.scan_answers(sw, policy)
        verdict = [es.in_policy(c.L, c.edits, policy) for c in sw.cases]
        inside = np.array([ok for ok, _ in verdict])
        planted = np.array([(c.entry, c.offset + policy[3], k) for c, (_, k) in zip(sw.cases, verdict)], dtype=np.int32)
        at_site = (scan == planted).all(axis=1)
        unaligned = (scan == -1).all(axis=1)
        # (the exact policies take the unedited reads only: one per site class and length)
        assert inside.sum() >= 10 * len(ws.lengths_of(W)) and (~inside).sum() > 100, (W, policy)
        f_in, f_out = at_site[inside].mean(), unaligned[~inside].mean()
        print("w%d %s: %d reads, in-policy at the planted site %.4f (%d), out-of-policy unaligned %.4f (%d)" %
              (W, policy, len(sw.cases), f_in, inside.sum(), f_out, (~inside).sum()))
        assert f_in >= 0.99 and f_out >= 0.99, (W, policy, f_in, f_out)
        moved = inside & ~at_site
        assert (scan[moved, 2] <= planted[moved, 2]).all() and (scan[moved, 2] >= 0).all(), (W, policy)


@pytest.fixture(scope="module")
def view(native_lib, sweeps):
    from mirge_amd.index import FmIndex
    sw = sweeps["w2"]
    return FmIndex.build(sw.names, sw.seqs).view()


@pytest.mark.parametrize("W", WORDS)
def test_the_port_equals_the_scan(sweeps, view, W):
    """model.fm_cascade (ftab, the default wstop) as a single-pass cascade against the scan, per policy: the batch with
    its N mask, `pair_anchor` 0 and -- the 2-mismatch policy -- 4 as the GPU reports it; the poly-T class under `poly_t`
    = 1.  Entry, offset and mismatches of every read, the processed / aligned counters."""
    for name, poly_t in (("w%d" % W, 0), ("w%d_polyt" % W, 1)):
        sw = sweeps[name]
        words, lens, nmask = ws.pack(sw)
        assert words.shape[0] == W and nmask is not None
        for policy in es.POLICIES:
            scan, processed = ws.scan_answers(sw, policy, poly_t)
            for pair_anchor in ((0, 4) if policy[1] == 2 and not poly_t else (0,)):
                p = dict(ws.pass_dict(policy, poly_t=poly_t), pair_anchor=pair_anchor)
                ref = model.fm_cascade([view], [p], words, lens, nmask, wstop=DEFAULT_WSTOP, ftab=True)
                got = es.claimed(ref["pass_id"], ref["ref_id"], ref["pos"], ref["mm"], 0)
                report = es.grid_report("CPU port (pair_anchor %d, poly_t %d) on %s" % (pair_anchor, poly_t, name), policy, sw.cases, got, scan)
                assert not report, report
                assert set(np.unique(ref["pass_id"]).tolist()) <= {0, -1}
                aligned = int((scan[:, 0] >= 0).sum())
                assert (int(ref["stats"][0][0]), int(ref["stats"][0][1])) == (processed, aligned), (name, policy)
                assert aligned > 10, (name, policy)      # (the comparison is not one of "nothing aligns" with itself)
