"""CPU side of the hand-made tally inputs (tests/tally_cases.py): the enumerated reads reach the branches they were
made for, and oracle/edit_tally.c -- the reference of tests/test_gpu_tally_kernels.py -- agrees on them with the
Python host path (a2i.a2i_editing, pinned to the reference's own output files by tests/golden/a2i.json)."""
import functools
import io

import numpy as np
import pytest

from mirge_amd import a2i
from oracle import model
from tests import tally_cases as tc


def kept_by_oracle(reads, **kw):
    """Per read: does oracle/edit_tally.c keep it?  (seq_true of runs that hold one read per entry.)"""
    lib = reads.lib
    kept = np.zeros(reads.n, bool)
    mirna = np.nonzero(reads.variant >= 0)[0]
    by_entry = [mirna[reads.ref_id[mirna] == e] for e in range(lib.n)]
    for g in range(max(len(x) for x in by_entry)):
        idx = np.array([x[g] for x in by_entry if g < len(x)])
        nm = None if reads.nmask is None else reads.nmask[:, idx]
        got = model.edit_tally(lib.index, reads.pass_id[idx], reads.ref_id[idx], reads.pos[idx], reads.words[:, idx],
                               reads.lens[idx], np.ones((len(idx), 1), np.uint32), nmask=nm, flank5=lib.flank5,
                               flank3=lib.flank3, **kw)
        kept[idx] = got[:lib.n * 3].reshape(lib.n, 3)[reads.ref_id[idx], 1] == 1
    return kept


@pytest.fixture(scope="module")
def standard(native_lib, oracle_lib):
    lib = tc.standard_library()
    reads = tc.enumerate_reads(lib)
    return lib, reads, kept_by_oracle(reads)


def test_libraries_are_what_the_cases_need(native_lib):
    lib = tc.standard_library()
    assert sorted(len(m) for m in lib.matures) == [1, 4, 5, 6] + list(range(18, 27)) + [32]
    for a, b, c in ((lib, 2, 6), (tc.flank_library(12, 0), 12, 0), (tc.flank_library(0, 9), 0, 9)):
        assert all(len(s) == b + len(m) + c and s[b:b + len(m)] == m for s, m in zip(a.seqs, a.matures))
        assert max(len(s) for s in a.seqs) <= 32 + b + c and a.index.n_ref == a.n
    ed = tc.edit_site_library()
    assert ed.n >= 256
    sites = {(e, i) for e, m in enumerate(ed.matures) for i in range(len(m) - 5) if m[i] == "A"}
    assert all(sum(m[i] == "A" for i in range(len(m) - 5)) >= 16 for m in ed.matures) and len(sites) >= 4096
    r = tc.edit_site_reads(ed, 4096)
    assert len(tc.edit_keys(r, 1)) == 4096 and len(tc.edit_keys(tc.edit_site_reads(ed, 1024), 3)) == 3072


def test_enumeration_covers_every_class(standard):
    lib, reads, kept = standard
    mi = reads.variant >= 0
    L = reads.lens.astype(np.int64)
    for e, m in enumerate(lib.matures):
        Lm = len(m)
        sel = mi & (reads.ref_id == e)
        assert set(reads.d[sel]) == set(range(-2, 4))
        assert set(L[sel]) == set(range(max(1, Lm - 6), min(40, Lm + 8) + 1))
        assert set(reads.pass_id[sel]) == {tc.CANON, tc.ISO}
        want = set(range(12)) if Lm >= 18 else {0, 4}
        assert want <= set(reads.variant[sel]), (Lm, sorted(set(reads.variant[sel])))
    iso = mi & (reads.pass_id == tc.ISO)
    assert np.array_equal(reads.pos[iso], 2 + reads.d[iso] + 1) and np.array_equal(reads.pos[mi & ~iso], 2 + reads.d[mi & ~iso])
    assert reads.words.shape[0] == 2 and int(L.max()) == 40                      # two-word reads occur
    other = ~mi & (reads.pass_id > 0)
    assert other.sum() > 100 and int(reads.ref_id[other].max()) > 150_000 and int((reads.pass_id == -1).sum()) > 100
    assert int((reads.quant(1) == 0).sum()) > 100 and reads.nmask is not None


def test_oracle_keeps_and_rejects_what_the_cases_aim_at(standard):
    lib, reads, kept = standard
    mi = reads.variant >= 0
    assert kept[mi].sum() >= mi.sum() / 4 and (~kept[mi]).sum() >= mi.sum() / 4
    assert not kept[~mi].any()
    Lm = np.array([len(m) for m in lib.matures])[np.where(mi, reads.ref_id, 0)]
    over = reads.d + reads.lens.astype(np.int64) - Lm                               # bases past the mature end
    for d in (-1, 0, 1):
        assert kept[mi & (reads.d == d)].any(), d
    assert not kept[mi & (reads.d > 1)].any()
    for k in (1, 2, 3):
        assert kept[mi & (over == k)].any(), k
    canonical = np.array([v >= 0 and s in lib.matures[e] for s, e, v in zip(reads.seqs, reads.ref_id, reads.variant)])
    assert (kept & canonical).any() and (kept & ~canonical & mi).any()
    for name in ("two_subs_judged",):
        assert not kept[reads.variant == tc.VARIANTS.index(name)].any()
    for name in ("sub_first_judged", "sub_last_judged", "sub_first_unjudged", "sub_past_end", "sub_judged_and_unjudged",
                 "edit_last_scored", "edit_scored", "edit_first_unscored", "n_on_scored_a", "n_elsewhere"):
        v = reads.variant == tc.VARIANTS.index(name)
        assert kept[v].any() and (~kept[v]).any(), name
    # the position table: a hit at the last scored position (Lm - 6), none at the first unscored one although kept
    # reads show a G there, none from an N on an edit site
    S = 1
    tab = model.edit_tally(lib.index, reads.pass_id, reads.ref_id, reads.pos, reads.words, reads.lens, reads.quant(S),
                           nmask=reads.nmask)
    per_pos = tab[lib.n * 3:].reshape(lib.n, 32)
    for e, m in enumerate(lib.matures):
        assert not per_pos[e, max(len(m) - 5, 0):].any()
        if len(m) >= 6:
            assert per_pos[e, len(m) - 6] > 0
    assert kept[reads.variant == tc.VARIANTS.index("edit_first_unscored")].any()


@pytest.mark.parametrize("flanks", [(2, 6), (12, 0), (0, 9)])
def test_c_restatement_equals_the_python_host_path_on_the_cases(native_lib, oracle_lib, monkeypatch, flanks):
    """oracle/edit_tally.c against a2i.a2i_editing, entry by entry, on the enumerated reads whose own best local
    alignment (a2i.local_pair) is the diagonal the case gives them -- the selection rule of
    test_edit_tally.py::test_c_restatement_equals_the_python_host_path.  A read that does not overlap the mature
    sequence at all, or has no local alignment with it whatever the diagonal (local_pair raises: the one base of a
    1-nt mature substituted), has no such diagonal: those are left out of the count, and of the others at least 90 %
    of every entry's reads must be selected."""
    monkeypatch.setattr(a2i, "local_pair", functools.lru_cache(maxsize=None)(a2i.local_pair))
    lib = tc.standard_library() if flanks == (2, 6) else tc.flank_library(*flanks)
    reads = tc.enumerate_reads(lib, extras=False)
    quant = reads.quant(1)
    quant[quant == 0] = 9
    M = lib.n
    L = reads.lens.astype(np.int64)
    seen_hits = 0
    for e, m in enumerate(lib.matures):
        idx = np.nonzero(reads.ref_id == e)[0]
        overlap = [i for i in idx if reads.d[i] < len(m) and reads.d[i] + L[i] > 0]
        sel, no_alignment = [], 0
        for i in overlap:
            try:
                tpad, spad = a2i.local_pair(m, reads.seqs[i])
            except ValueError:
                no_alignment += 1      # (the read shares no base with the mature sequence: a 1-nt mature, substituted)
                continue
            if a2i.dash_count(spad)[0] - a2i.dash_count(tpad)[0] == reads.d[i]:
                sel.append(i)
        assert len(sel) >= 0.9 * (len(overlap) - no_alignment), (len(m), len(sel), len(overlap), no_alignment)
        keep = np.zeros(reads.n, np.uint8)
        keep[sel] = 1
        one = model.edit_tally(lib.index, reads.pass_id, reads.ref_id, reads.pos, reads.words, reads.lens, quant,
                               nmask=reads.nmask, keep=keep, flank5=lib.flank5, flank3=lib.flank3)
        rs = [reads.seqs[i] for i in sel]
        cs = [int(quant[i, 0]) for i in sel]
        _, positions, pos_count, _, _, count_true, seq_true, canonical = a2i.a2i_editing(m, rs, cs, lib.names[e], io.StringIO(),
                                                                                         set(rs))
        assert (int(one[e * 3]), int(one[e * 3 + 1]), int(one[e * 3 + 2])) == (count_true, seq_true, canonical), len(m)
        want = np.zeros(32, np.int64)
        for p in positions:
            want[p - 1] = pos_count[p]
        assert np.array_equal(one[M * 3:].reshape(M, 32)[e].astype(np.int64), want), len(m)
        assert seq_true > 0
        seen_hits += int(want.sum() > 0)
    assert seen_hits >= sum(len(m) >= 6 for m in lib.matures)
