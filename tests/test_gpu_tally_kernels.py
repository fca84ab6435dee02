"""tally_kernel and edit_tally_kernel on the hand-made inputs of tests/tally_cases.py, against oracle/edit_tally.c
and oracle/fm_cpu.c's orc_tally, for exact equality.  Every run writes into a zeroed slice between two guard
stretches of a larger tensor, is repeated into the same slice (counts accumulate: exactly twice the reference),
and states which instantiation it expects; mrg_ctx_last_tally_launch says which one answered.  The expectation
is worked out here from the launchers' rules (csrc/capi.hip: tally_run_impl, edit_tally_impl)."""
import numpy as np
import pytest

from mirge_amd._native import MirgeAmdError
from oracle import model
from tests import tally_cases as tc

pytestmark = pytest.mark.gpu

GUARD, SENTINEL = 96, 0x5A5A5A5A5A5A5A5A
LDS_DEFAULT = 160 * 1024
HASH_BYTES = 24576                      # kEditHashLdsBytes: 2048 slots of a 4-byte key and an 8-byte sum
THREADS = 1024                          # kTallyThreads = kEditThreads
CAT_REPLICAS = 32                       # kTallyCatReplicas


@pytest.fixture(scope="module")
def world(native_lib, oracle_lib):
    from mirge_amd.engine import Engine
    eng = Engine(0)
    libs = dict(std=tc.standard_library(), f12=tc.flank_library(12, 0), f9=tc.flank_library(0, 9), sites=tc.edit_site_library())
    for k, lib in libs.items():
        eng.add_library(k, lib.index)
    cache = {}

    def reads_of(key, trim=1):
        if (key, trim) not in cache:
            cache[key, trim] = tc.enumerate_reads(libs[key], trim=trim)
        return cache[key, trim]
    yield eng, libs, reads_of
    eng.set_option("lds_budget", LDS_DEFAULT)
    eng.close()


# ---------------------------------------------------------------------------------------------- plumbing
_SIGNED = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32}


def up(eng, a, off=False):
    """A host array on the device, as the flat buffer the kernels index.  off: one element into a larger buffer, so
    that the pointer is aligned to its element size and to nothing wider."""
    import torch
    a = np.ascontiguousarray(a)
    a = a.view(_SIGNED.get(a.dtype, a.dtype))
    t = torch.from_numpy(a).to(eng.device)
    if off:
        buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=eng.device)
        buf[1:].copy_(t.reshape(-1))
        t = buf[1:].view(t.shape)
        assert t.data_ptr() % 16 != 0 and (t.element_size() >= 4 or t.data_ptr() % 4 != 0)
    return t


def guarded(eng, ln):
    import torch
    big = torch.full((GUARD + ln + GUARD,), SENTINEL, dtype=torch.int64, device=eng.device)
    big[GUARD:GUARD + ln] = 0
    return big, big[GUARD:GUARD + ln]


def read_back(big, ln):
    h = big.cpu().numpy()
    assert (h[:GUARD] == SENTINEL).all() and (h[GUARD + ln:] == SENTINEL).all(), "the launch wrote outside its counts"
    return h[GUARD:GUARD + ln].view(np.uint64).copy()


def assignment(eng, pass_id, ref_id, pos, n_pass, packed, off):
    from mirge_amd.engine import CascadeResult
    off = set(off)
    res = CascadeResult(up(eng, pass_id, "pass" in off and not packed), up(eng, ref_id, "ref" in off and not packed),
                        up(eng, pos, "pos" in off and not packed), up(eng, np.zeros(len(pass_id), np.uint8)), None, eng, n_pass)
    if not packed:
        return res
    pk = eng.pack_assignments(res)
    if off & {"pass", "ref", "pos", "packed"}:
        pk = up(eng, pk.cpu().numpy(), True)
    return CascadeResult(None, None, None, None, None, eng, n_pass, packed=pk)


ALL_OFF = ("reads", "lens", "pass", "ref", "pos", "quant")


def run_edit(eng, key, reads, quant, packed=False, keep=None, remap=None, n_bins=None, off=(), nmask="own", **kw):
    """Engine.edit_tally on hand-made arrays, twice into one guarded slice.  Returns (counts, launch record)."""
    from mirge_amd.engine import ReadSet
    nm = reads.nmask if isinstance(nmask, str) else nmask
    rs = ReadSet.from_device(up(eng, reads.words, "reads" in off), up(eng, reads.lens, "lens" in off),
                             None if nm is None else up(eng, nm), up(eng, quant, "quant" in off))
    res = assignment(eng, reads.pass_id, reads.ref_id, reads.pos, 9, packed, off)
    ln = eng.edit_counts_len(key, quant.shape[1], n_bins)
    big, out = guarded(eng, ln)
    args = dict(lib=key, counts=out, keep=None if keep is None else up(eng, keep),
                remap=None if remap is None else up(eng, remap.astype(np.int32)), n_bins=n_bins, **kw)
    eng.edit_tally(rs, res, **args)
    launch = eng.last_tally_launch(edit=True)
    once = read_back(big, ln)
    eng.edit_tally(rs, res, **args)
    assert eng.last_tally_launch(edit=True) == launch
    twice = read_back(big, ln)
    assert np.array_equal(twice, 2 * once), "a second launch into the same counts did not add the same again"
    return once, launch


def edit_want(reads, quant, nmask="own", **kw):
    lib = reads.lib
    nm = reads.nmask if isinstance(nmask, str) else nmask
    return model.edit_tally(lib.index, reads.pass_id, reads.ref_id, reads.pos, reads.words, reads.lens, quant, nmask=nm,
                            flank5=lib.flank5, flank3=lib.flank3, **kw)


def hist_bytes(n_bins, S):
    """edit_hist_lds_bytes (csrc/kernels.hpp)."""
    return n_bins * S * 16 + ((n_bins * S + 3) & ~3) * 4


def lib_bytes(index):
    text_words = (int(index.info.text_words) + 3) // 4 * 4
    return text_words * 4 + ((index.n_ref + 4) & ~3) * 4


def expect_edit(eng, index, n_bins, S, lds_budget, n, vec4):
    """edit_tally_impl's choice: the totals go to LDS when they fit the budget left by the hash, the library too when
    all of it fits min(that, 80 KiB)."""
    budget = max(lds_budget, HASH_BYTES) - HASH_BYTES
    h = hist_bytes(n_bins, S)
    lds_hist = h <= budget
    lds_lib = (h if lds_hist else 0) + lib_bytes(index) + HASH_BYTES <= min(budget, 80 * 1024)
    lds = (h if lds_hist else 0) + (lib_bytes(index) if lds_lib else 0) + HASH_BYTES
    want = ((n + 3) // 4 if vec4 else n) + THREADS - 1
    grid = min(want // THREADS, eng.n_cu * (2 if lds * 2 <= 160 * 1024 else 1))
    return dict(lds_hist=lds_hist, lds_lib=lds_lib, vec4=vec4, grid=grid, lds_bytes=lds)


def edit_setting(index, inst):
    """(lds_budget, samples) that make edit_tally_impl choose instantiation <lds_hist, lds_lib> for this library
    with one bin per entry (64 entries: default / 40000 / 60000 with 28 samples / 0 fall in the same ranges)."""
    n = index.n_ref
    if inst == (True, True):
        return LDS_DEFAULT, 1
    if inst == (True, False):
        return HASH_BYTES + hist_bytes(n, 1), 1          # the totals fit exactly: nothing is left for the library
    if inst == (False, False):
        return 0, 1
    S = 1
    while hist_bytes(n, S) <= lib_bytes(index) + HASH_BYTES:
        S += 1
    return 2 * HASH_BYTES + lib_bytes(index), S          # the library fits exactly; the totals of S samples do not


INSTANTIATIONS = [(True, True), (True, False), (False, True), (False, False)]


# ---------------------------------------------------------------------------------------------- edit tally
@pytest.mark.parametrize("inst", INSTANTIATIONS, ids=lambda i: "hist%d-lib%d" % i)
@pytest.mark.parametrize("key", ["std", "f12", "f9"])
def test_edit_enumerated_reads_in_every_instantiation(world, key, inst):
    eng, libs, reads_of = world
    lib, reads = libs[key], reads_of(key)
    budget, S = edit_setting(lib.index, inst)
    quant = reads.quant(S)
    keep = (np.arange(reads.n) % 3 != 0).astype(np.uint8)
    remap = (np.arange(lib.n) // 2).astype(np.uint32)
    nb2 = int(remap.max()) + 1
    fl = dict(flank5=lib.flank5, flank3=lib.flank3)
    eng.set_option("lds_budget", budget)
    try:
        for packed, kp, rm in ((False, None, None), (True, None, None), (False, keep, None), (True, keep, remap),
                               (False, None, remap)):
            nb = lib.n if rm is None else nb2
            # (merged bins change the size of the totals: the library still fits, and whether the totals do is worked out)
            exp = expect_edit(eng, lib.index, nb, S, budget, reads.n, False)
            if rm is None:
                assert (exp["lds_hist"], exp["lds_lib"]) == inst
            got, launch = run_edit(eng, key, reads, quant, packed=packed, keep=kp, remap=rm, n_bins=None if rm is None else nb, **fl)
            assert launch == exp, (packed, kp is not None, rm is not None)
            want = model.edit_tally(lib.index, reads.pass_id, reads.ref_id, reads.pos, reads.words, reads.lens, quant,
                                    nmask=reads.nmask, keep=kp, remap=rm, n_bins=None if rm is None else nb, **fl)
            assert np.array_equal(got, want), (packed, kp is not None, rm is not None)
            assert int(want[:nb * S * 3].sum()) > 0 and int(want[nb * S * 3:].sum()) > 0
    finally:
        eng.set_option("lds_budget", LDS_DEFAULT)


def test_edit_other_substitution_and_other_trim(world):
    eng, libs, reads_of = world
    reads = reads_of("std")
    quant = reads.quant(3)
    got, _ = run_edit(eng, "std", reads, quant, from_base=1, to_base=3)                      # C -> T
    want = edit_want(reads, quant, from_base=1, to_base=3)
    assert np.array_equal(got, want) and not np.array_equal(want, edit_want(reads, quant))
    # G -> A: a packed N carries base code 0 = A and must not read as the A of an edit (with any other `to_base`
    # the code alone keeps it out); without the mask the same reads do count there
    got, _ = run_edit(eng, "std", reads, quant, from_base=2, to_base=0)
    want = edit_want(reads, quant, from_base=2, to_base=0)
    k = reads.lib.n * 3 * 3
    assert np.array_equal(got, want)
    assert not np.array_equal(want[k:], edit_want(reads, quant, nmask=None, from_base=2, to_base=0)[k:])
    r3 = reads_of("std", trim=3)                                                            # isomiR pass: `-5 3`
    for packed in (False, True):
        got, _ = run_edit(eng, "std", r3, quant, packed=packed, isomir_trim5=3)
        want = edit_want(r3, quant, isomir_trim5=3)
        assert np.array_equal(got, want) and not np.array_equal(want, edit_want(r3, quant, isomir_trim5=1))


def one_word_subset(reads, n):
    """n one-word reads of an enumeration, strided through it; the first one and the n % 4 last ones (the reads
    that are never taken four at a time) are kept reads with an edit."""
    ow = np.nonzero(reads.lens <= 32)[0]
    Lm = np.array([len(m) for m in reads.lib.matures])[np.where(reads.variant >= 0, reads.ref_id, 0)]
    edited = np.nonzero((reads.variant[ow] == tc.VARIANTS.index("edit_scored")) & (reads.d[ow] == 0) &
                        (reads.lens[ow] == Lm[ow]) & (Lm[ow] >= 18))[0]
    at = (edited[1] + np.arange(n) * 37) % len(ow)
    at[n - n % 4:] = edited[2:2 + n % 4]
    return tc.Reads(reads.lib, [(reads.seqs[i], reads.pass_id[i], reads.ref_id[i], reads.pos[i], reads.d[i], reads.variant[i])
                                for i in ow[at]], 1)


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 4096, 4099])
def test_edit_vec4_and_scalar_tail(world, n):
    """One sample, one-word reads: four reads per lane where every pointer allows 16-byte loads, the n % 4 reads left
    one by one; the same arrays one element into a larger buffer must take the scalar path and count the same."""
    eng, libs, reads_of = world
    sub = one_word_subset(reads_of("std"), n)
    quant = sub.quant(1)
    quant[0] = 2
    want = edit_want(sub, quant)
    assert int(want[:libs["std"].n * 3].sum()) > 0 and int(want[libs["std"].n * 3:].sum()) > 0
    for packed in (False, True):
        got, launch = run_edit(eng, "std", sub, quant, packed=packed)
        assert launch == expect_edit(eng, sub.lib.index, sub.lib.n, 1, LDS_DEFAULT, n, True)
        assert np.array_equal(got, want)
        got, launch = run_edit(eng, "std", sub, quant, packed=packed, off=ALL_OFF)
        assert launch == expect_edit(eng, sub.lib.index, sub.lib.n, 1, LDS_DEFAULT, n, False)
        assert np.array_equal(got, want)
    # a keep mask and merged bins on the four-per-lane path, with the library gathered from HBM (<true, false>)
    lib = sub.lib
    keep = (np.arange(n) % 3 != 1).astype(np.uint8)
    remap = (np.arange(lib.n) // 2).astype(np.uint32)
    nb = int(remap.max()) + 1
    budget = HASH_BYTES + hist_bytes(nb, 1)
    want_kr = edit_want(sub, quant, keep=keep, remap=remap, n_bins=nb)
    assert n < 1000 or (not np.array_equal(want_kr, edit_want(sub, quant, remap=remap, n_bins=nb)) and int(want_kr.sum()) > 0)
    eng.set_option("lds_budget", budget)
    try:
        for packed in (False, True):
            got, launch = run_edit(eng, "std", sub, quant, packed=packed, keep=keep, remap=remap, n_bins=nb)
            assert launch == expect_edit(eng, lib.index, nb, 1, budget, n, True)
            assert (launch["lds_hist"], launch["lds_lib"], launch["vec4"]) == (True, False, True)
            assert np.array_equal(got, want_kr), packed
    finally:
        eng.set_option("lds_budget", LDS_DEFAULT)
    if n == 4099:   # each pointer on its own decides too; without an N mask, and without the library in LDS
        for which in ALL_OFF + ("packed",):
            got, launch = run_edit(eng, "std", sub, quant, packed=which == "packed", off=(which,))
            assert not launch["vec4"] and np.array_equal(got, want), which
        clean = sub.take(np.nonzero(sub.nmask[0] == 0)[0])
        eng.set_option("lds_budget", 0)
        try:
            got, launch = run_edit(eng, "std", clean, clean.quant(1), nmask=None)
            assert launch == expect_edit(eng, sub.lib.index, sub.lib.n, 1, 0, clean.n, True) and not launch["lds_hist"]
            assert np.array_equal(got, edit_want(clean, clean.quant(1), nmask=None))
        finally:
            eng.set_option("lds_budget", LDS_DEFAULT)


@pytest.mark.parametrize("with_n", [True, False])
def test_edit_two_word_reads(world, with_n):
    eng, libs, reads_of = world
    reads = reads_of("std")
    has_n = (reads.nmask != 0).any(axis=0)
    long_ = np.nonzero((reads.lens >= 33) & (with_n | ~has_n))[0]
    near = np.nonzero((reads.lens >= 27) & (reads.lens <= 32) & ~has_n)[0][:500]
    sub = reads.take(np.sort(np.concatenate([long_, near])))
    assert sub.words.shape[0] == 2 and set(range(33, 41)) <= set(sub.lens) and (sub.nmask is not None) == with_n
    for S in (1, 3):
        quant = sub.quant(S)
        want = edit_want(sub, quant)
        assert int(want[sub.lib.n * S * 3:].sum()) > 0
        for packed in (False, True):
            got, launch = run_edit(eng, "std", sub, quant, packed=packed)
            assert not launch["vec4"] and np.array_equal(got, want)


@pytest.mark.parametrize("S,n", [(3, 1024), (1, 4096)], ids=["scalar", "vec4"])
def test_edit_hash_overflow(world, S, n):
    """One workgroup, more distinct (bin, position, sample) keys than its 2048-slot LDS hash has slots: whatever
    the probe order, some keys find four occupied slots and must go to the global array directly."""
    eng, libs, _ = world
    lib = libs["sites"]
    reads = tc.edit_site_reads(lib, n)
    quant = 1 + (np.arange(n * S, dtype=np.uint32).reshape(n, S) % 7)
    assert len(tc.edit_keys(reads, S)) == n * S > 2048
    want = edit_want(reads, quant)
    per_pos = want[lib.n * S * 3:]
    assert int((per_pos != 0).sum()) == n * S and int(per_pos.sum()) == int(quant.sum())
    for packed in (False, True):
        got, launch = run_edit(eng, "sites", reads, quant, packed=packed)
        assert launch["grid"] == 1 and launch["vec4"] == (S == 1)
        assert launch == expect_edit(eng, lib.index, lib.n, S, LDS_DEFAULT, n, S == 1)
        assert np.array_equal(got, want)


@pytest.mark.parametrize("S", [1, 3])
def test_edit_hot_key_sums_past_32_bits(world, S):
    eng, libs, _ = world
    lib = libs["sites"]
    reads = tc.edit_site_reads(lib, 1).take(np.zeros(1024, np.int64))     # 1024 times entry 0 with its first A edited
    assert len(set(reads.seqs)) == 1 and len(tc.edit_keys(reads, S)) == S
    quant = np.full((1024, S), 0xFFFFFFFF, np.uint32)
    want = edit_want(reads, quant)
    site = [i for i, c in enumerate(lib.matures[0]) if c == "A"][0]
    tot, per_pos = want[:lib.n * S * 3].reshape(lib.n, S, 3), want[lib.n * S * 3:].reshape(lib.n, 32, S)
    assert (tot[0, :, 0] == 1024 * 0xFFFFFFFF).all() and (tot[0, :, 1] == 1024).all() and (tot[0, :, 2] == 0).all()
    assert (per_pos[0, site] == 1024 * 0xFFFFFFFF).all() and int(per_pos.sum()) == S * 1024 * 0xFFFFFFFF > 2 ** 32
    for budget in (LDS_DEFAULT, 0):
        eng.set_option("lds_budget", budget)
        try:
            got, launch = run_edit(eng, "sites", reads, quant)
            assert launch == expect_edit(eng, lib.index, lib.n, S, budget, 1024, S == 1)
            assert np.array_equal(got, want)
        finally:
            eng.set_option("lds_budget", LDS_DEFAULT)


def test_last_launch_query_arguments(world):
    import ctypes as C
    eng = world[0]
    out = (C.c_uint32 * 4)()
    for which in (-1, 2):
        assert eng._lib.mrg_ctx_last_tally_launch(eng._h, which, out) < 0 and b"which" in eng._lib.mrg_last_error()
    assert eng._lib.mrg_ctx_last_tally_launch(eng._h, 0, None) < 0 and b"null" in eng._lib.mrg_last_error()
    assert eng._lib.mrg_ctx_last_tally_launch(eng._h, 1, out) == 0 and out[3] == 0


def test_edit_argument_errors(world):
    eng, libs, reads_of = world
    sub = one_word_subset(reads_of("std"), 16)
    quant = sub.quant(1)
    _, before = run_edit(eng, "std", sub, quant)
    with pytest.raises(MirgeAmdError, match="bases"):
        run_edit(eng, "std", sub, quant, from_base=2, to_base=2)
    with pytest.raises(MirgeAmdError, match="no remap"):
        run_edit(eng, "std", sub, quant, n_bins=libs["std"].n + 1)
    with pytest.raises(MirgeAmdError, match="longer than"):
        run_edit(eng, "std", sub, quant, flank5=0, flank3=0)
    assert eng.last_tally_launch(edit=True) == before         # a refused call is no launch
    got, _ = run_edit(eng, "std", sub, quant)                 # (and the engine still counts afterwards)
    assert np.array_equal(got, edit_want(sub, quant))


# ---------------------------------------------------------------------------------------------- tally
def expect_tally(eng, M, S, n_pass, lds_budget, n, vec4):
    bins = 2 * M * S + (n_pass + 1) * S + S
    lds = (bins + (n_pass + 1) * S * (CAT_REPLICAS - 1)) * 8
    lds_hist = lds <= lds_budget
    want = (((n + 3) // 4 if vec4 else n) + THREADS - 1) // THREADS
    per_cu = (2 if lds * 2 <= 160 * 1024 else 1) if lds_hist else 2
    return dict(lds_hist=lds_hist, lds_lib=False, vec4=vec4, grid=min(want, eng.n_cu * per_cu), lds_bytes=lds if lds_hist else 0)


def run_tally(eng, pass_id, ref_id, quant, M, n_pass, canon, iso, packed=False, off=()):
    from mirge_amd.engine import ReadSet
    n, S = quant.shape
    rs = ReadSet.from_device(up(eng, np.zeros((1, n), np.uint64)), up(eng, np.zeros(n, np.uint8)), None, up(eng, quant, "quant" in off))
    res = assignment(eng, pass_id, ref_id, np.where(pass_id < 0, -1, 0).astype(np.int32), n_pass, packed, off)
    ln = eng.counts_len(M, S, n_pass)
    big, out = guarded(eng, ln)
    eng.tally(rs, res, M, canon_pass=canon, isomir_pass=iso, counts=out)
    launch = eng.last_tally_launch()
    once = read_back(big, ln)
    eng.tally(rs, res, M, canon_pass=canon, isomir_pass=iso, counts=out)
    twice = read_back(big, ln)
    assert np.array_equal(twice, 2 * once), "a second launch into the same counts did not add the same again"
    return once, launch


TALLY_N = [1, 2, 3, 4, 5, 1023, 4097, 4 * 1024 * 3 + 1]


@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("n_pass", [1, 9, 15])
@pytest.mark.parametrize("M", [7, 300])
def test_tally_sizes_forms_and_alignment(world, M, n_pass, S):
    eng = world[0]
    canon, iso = 0, (n_pass - 1 if n_pass > 1 else -1)
    seen = set()
    for n in TALLY_N:
        pass_id, ref, quant = tc.tally_content(n, M, n_pass, canon, iso, S)
        want = model.tally(pass_id, ref, quant, M, n_pass, canon, iso)
        assert int(want.sum()) > 0
        for budget in (LDS_DEFAULT, 0):
            eng.set_option("lds_budget", budget)
            try:
                for packed in (False, True):
                    for off in ((), ("pass", "ref", "quant")):
                        vec4 = S == 1 and not off
                        got, launch = run_tally(eng, pass_id, ref, quant, M, n_pass, canon, iso, packed, off)
                        assert launch == expect_tally(eng, M, S, n_pass, budget, n, vec4), (n, budget, packed, off)
                        assert launch["lds_hist"] == (budget != 0)
                        assert np.array_equal(got, want), (n, budget, packed, off)
                        seen.add((launch["lds_hist"], launch["vec4"]))
            finally:
                eng.set_option("lds_budget", LDS_DEFAULT)
        if S == 1 and n == 4097:   # each pointer on its own
            for which in ("pass", "ref", "quant", "packed"):
                got, launch = run_tally(eng, pass_id, ref, quant, M, n_pass, canon, iso, which == "packed", (which,))
                assert not launch["vec4"] and np.array_equal(got, want), which
    assert seen == ({(True, True), (False, True), (True, False), (False, False)} if S == 1 else {(True, False), (False, False)})


@pytest.mark.parametrize("S", [1, 3])
def test_tally_mixed_content_and_counts_near_2_to_32(world, S):
    """Unclaimed reads, reads of other passes with entry numbers far above M, zero counts, and 300 reads of one
    miRNA plus 300 of one category with 2^32 - 1 in every sample: the bins are 64-bit everywhere."""
    eng = world[0]
    M, n_pass, canon, iso, n = 300, 9, 0, 8, 4097
    pass_id, ref, quant = tc.tally_content(n, M, n_pass, canon, iso, S, big=300)
    other = (pass_id > 0) & (pass_id < 8)
    assert int(ref[other].max()) > 150_000 and int((pass_id == -1).sum()) > 100 and int((quant == 0).all(axis=1).sum()) > 100
    want = model.tally(pass_id, ref, quant, M, n_pass, canon, iso)
    q, iscan, cat, uniq = (want[:M * S].reshape(M, S), want[M * S:2 * M * S].reshape(M, S),
                           want[2 * M * S:2 * M * S + (n_pass + 1) * S].reshape(n_pass + 1, S), want[-S:])
    assert (q[1] >= 300 * 0xFFFFFFFF).all() and (iscan[1] >= 300 * 0xFFFFFFFF).all() and (cat[8] >= 300 * 0xFFFFFFFF).all()
    assert (uniq == (quant != 0).sum(axis=0)).all() and (uniq < n).all()
    claimed = (pass_id == canon) | (pass_id == iso)
    assert int(q.sum()) == int(quant[claimed].astype(np.uint64).sum())       # nothing else reaches the miRNA bins
    for budget in (LDS_DEFAULT, 0):
        eng.set_option("lds_budget", budget)
        try:
            for packed in (False, True):
                got, launch = run_tally(eng, pass_id, ref, quant, M, n_pass, canon, iso, packed)
                assert launch == expect_tally(eng, M, S, n_pass, budget, n, S == 1)
                assert np.array_equal(got, want), (budget, packed)
        finally:
            eng.set_option("lds_budget", LDS_DEFAULT)


@pytest.mark.parametrize("canon,iso", [(0, -1), (-1, 8), (-1, -1), (8, 8), (0, 14), (14, 0), (3, 3)])
def test_tally_pass_roles(world, canon, iso):
    """A disabled pass (-1) must not match the unclaimed reads' -1; one pass in both roles counts as canonical; the
    last pass can claim."""
    eng = world[0]
    M, n_pass, n = 7, 15, 1023
    for S in (1, 3):
        pass_id, ref, quant = tc.tally_content(n, M, n_pass, canon, iso, S)
        want = model.tally(pass_id, ref, quant, M, n_pass, canon, iso)
        assert (int(want[:M * S].sum()) > 0) == (canon >= 0 or iso >= 0) and int((pass_id == -1).sum()) > 30
        for budget in (LDS_DEFAULT, 0):
            eng.set_option("lds_budget", budget)
            try:
                for packed in (False, True):
                    got, _ = run_tally(eng, pass_id, ref, quant, M, n_pass, canon, iso, packed)
                    assert np.array_equal(got, want), (S, budget, packed)
            finally:
                eng.set_option("lds_budget", LDS_DEFAULT)
