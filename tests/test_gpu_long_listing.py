"""GPU (-m gpu): the listing for reads of any length (long_valid_kernel, mrg_list_valid_long_count / _fill,
Engine.list_valid_long) and the bowtie front end on reads beyond 255 nt.

The yardstick is tests/bowtie_text_model.py over oracle.model.list_valid (the exhaustive scan).  Every world is checked
twice: Engine.list_valid_long against the model, read by read and in the stated order; and the two C-ABI sweeps called
directly, with guard words behind every output buffer, `cap` a few rows short, muted reads (best_mm 255) and a second
fill into the same buffers.  Before anything is compared the model's own output must show that the world is not
empty: at least half of its reads beyond 255 nt align, one of them holds more than 64 alignments, one none."""
import numpy as np
import pytest

from tests import bowtie_text_model as btm
from tests.test_bowtie_cli import SHAPES, random_world, revcomp, rnd

pytestmark = pytest.mark.gpu

BIG_SEED = 1 << 20      # `-v`: the whole read is seed, however long it is
POLICIES = {"-n 0 -l 28": (28, 0, 2), "-n 0 -l 25": (25, 0, 2), "-n 1 -l 28": (28, 1, 2), "-n 1 -l 15": (15, 1, 2),
            "-v 0": (BIG_SEED, 0, 0), "-v 1": (BIG_SEED, 1, 1), "-v 2": (BIG_SEED, 2, 2)}
MORE_POLICIES = dict(POLICIES, **{"-n 2 -l 28": (28, 2, 2)})     # (K = 3 with a short seed)
PLANTS = (0, 1, 63, 64, 65, 130)     # copies of the 300-nt elements: the lane trips and the slot prefix
REP_COPIES = 1000
GUARD = 16
I32_GUARD, U8_GUARD = -0x5A5A5A5B, 0xEE


def sub(s, i, ch=None):
    """s with base i replaced (by another base, or by ch)."""
    return s[:i] + (ch or "ACGT"[("ACGT".index(s[i]) + 1) % 4]) + s[i + 1:]


class Planted:
    """Two parts: six entries of 300-1500 nt with N runs each (one of them without N, one pair whose boundary a read
    can straddle), and two carrier entries each that hold the planted copies on both strands: 300-nt elements with
    0, 1, 63, 64, 65 and 130 copies, and a 24-nt repeat with 1000 copies of which two continue as the read does."""

    def __init__(self, seed=11):
        rng = np.random.default_rng(seed)
        self.rng = rng
        self.elem = {c: rnd(rng, 300) for c in PLANTS}
        self.rep, self.rep_tail = rnd(rng, 24), rnd(rng, 276)
        items = []
        for c, e in self.elem.items():
            items += [e if i % 2 == 0 else revcomp(e) for i in range(c)]
        items += [self.rep + rnd(rng, 12) if i % 2 == 0 else revcomp(self.rep + rnd(rng, 12)) for i in range(REP_COPIES - 2)]
        items += [self.rep + self.rep_tail, revcomp(self.rep + self.rep_tail)]
        order = rng.permutation(len(items))
        carriers = [[] for _ in range(4)]
        for k, i in enumerate(order):
            carriers[k % 4] += [rnd(rng, int(rng.integers(3, 30))), items[i]]
            if rng.random() < 0.02:
                carriers[k % 4].append("N" * int(rng.integers(1, 40)))
        self.parts = []
        for p in range(2):
            names, seqs = [], []
            for e in range(6):
                s = rnd(rng, int(rng.integers(300, 1500)) if e else 1400)
                if e >= 2:     # (entries 0 and 1 stay free of N: the whole-entry read and the boundary read)
                    at = int(rng.integers(0, len(s) - 60))
                    s = s[:at] + "N" * int(rng.integers(1, 50)) + s[at:]
                names.append("p%de%d" % (p, e))
                seqs.append(s)
            for c in range(2):
                names.append("p%dcarrier%d" % (p, c))
                seqs.append("".join(carriers[2 * p + c]) + rnd(rng, 20))
            self.parts.append((names, seqs))
        self.world = btm.World(self.parts)
        self.longest = max(len(s) for _, ss in self.parts for s in ss)

    def entry(self, p, e):
        return self.parts[p][1][e]

    def draw(self, L, strand=0):
        """L bases without N of a random ordinary entry, on the given strand."""
        while True:
            p, e = int(self.rng.integers(0, 2)), int(self.rng.integers(0, 6))
            s = self.entry(p, e)
            if len(s) >= L:
                at = int(self.rng.integers(0, len(s) - L + 1))
                if "N" not in s[at:at + L]:
                    return revcomp(s[at:at + L]) if strand else s[at:at + L]


@pytest.fixture(scope="module")
def planted(native_lib, oracle_lib):
    from mirge_amd.engine import Engine
    from mirge_amd.index import FmIndex
    w = Planted()
    eng = Engine(0)
    w.keys = []
    for k, (names, seqs) in enumerate(w.parts):
        w.keys.append("part%d" % k)
        eng.add_library(w.keys[-1], FmIndex.build(names, seqs))
    w.eng = eng
    yield w
    eng.close()


def model_rows(world, reads, seed, cache):
    """Per read the model's [(mm, entry, offset, strand)] of every valid alignment on both strands."""
    out = []
    for q in reads:
        if (q, seed) not in cache:
            cache[(q, seed)] = world.hits(q, seed, False, 8192)
        out.append(cache[(q, seed)])
    return out


def reported(hits, strands, best, m=0):
    """What a mode lists of one read's hits, in the front end's order, and whether -m suppresses it."""
    hs = [h for h in hits if strands == 2 or h[3] == 0]
    if best and hs:
        lo = min(h[0] for h in hs)
        hs = [h for h in hs if h[0] == lo]
    if m and len(hs) > m:
        return [], True
    return sorted(hs, key=lambda h: (h[0], -h[1], -h[2], -h[3])), False


def assert_not_hidden(reads, hits):
    long_ = [h for q, h in zip(reads, hits) if len(q) > 255]
    assert long_, "no read beyond 255 nt"
    assert 2 * sum(1 for h in long_ if h) >= len(long_), "fewer than half of the long reads align in the model"
    assert any(len(h) > 64 for h in long_), "no long read with more than 64 alignments"
    assert any(not h for h in long_), "no unaligned long read"


def raw_listing(eng, lid, reads, strands, seed, best, mute=()):
    """The two sweeps through ctypes against ONE library: guards behind every buffer, a second fill into the same
    buffers, cap three rows short, the reads in `mute` given best_mm 255.  Returns per read [(mm, ref, pos, strand)]
    in slot order, and the counts [4, n]."""
    import torch
    from mirge_amd import pack
    from mirge_amd._native import check
    lib, dev, n = eng._lib, eng.device, len(reads)
    words, nmask, word_off, lens = pack.pack_ragged(list(reads))

    def up(a, dt):
        return torch.from_numpy(np.ascontiguousarray(a).view(dt)).to(dev)
    d_words = up(np.append(words, np.uint64(0)), np.int64)
    d_nmask = None if nmask is None else up(np.append(nmask, np.uint64(0)), np.int64)
    d_off, d_lens = up(word_off, np.int64), up(lens, np.int32)
    head = (eng._h, d_words.data_ptr(), None if d_nmask is None else d_nmask.data_ptr(), d_off.data_ptr(), d_lens.data_ptr(), n,
            lid, strands) + tuple(seed)
    cnt = torch.full((4 * n + GUARD,), I32_GUARD, dtype=torch.int32, device=dev)
    check(lib.mrg_list_valid_long_count(*head, cnt.data_ptr(), eng._stream_ptr()))
    c = cnt.cpu().numpy()
    assert (c[4 * n:] == I32_GUARD).all(), "count sweep wrote behind its buffer"
    counts = c[:4 * n].view(np.uint32).astype(np.int64).reshape(4, n)
    aligned = counts.any(axis=0)
    best_mm = np.where(aligned, np.argmax(counts > 0, axis=0), 255)
    best_mm[list(mute)] = 255
    k = np.where(best_mm == 255, 0, counts[np.minimum(best_mm, 3), np.arange(n)] if best else counts.sum(axis=0))
    off = np.zeros(n + 1, np.int64)
    np.cumsum(k, out=off[1:])
    t = int(off[-1])
    d_best, d_o = torch.from_numpy(best_mm.astype(np.uint8)).to(dev), torch.from_numpy(off).to(dev)

    def fill(cap, bufs=None):
        bufs = bufs or [torch.full((t + GUARD,), v, dtype=dt, device=dev) for v, dt in
                        ((I32_GUARD, torch.int32), (I32_GUARD, torch.int32), (U8_GUARD, torch.uint8), (U8_GUARD, torch.uint8))]
        check(lib.mrg_list_valid_long_fill(*head, 0 if best else 1, d_best.data_ptr(), d_o.data_ptr(), cap,
                                           *[b.data_ptr() for b in bufs], eng._stream_ptr()))
        torch.cuda.current_stream(dev).synchronize()
        return bufs, [b.cpu().numpy() for b in bufs]
    bufs, full = fill(t)
    for a, g in zip(full, (I32_GUARD, I32_GUARD, U8_GUARD, U8_GUARD)):
        assert (a[t:] == g).all(), "fill sweep wrote behind its buffer"
    _, again = fill(t, bufs)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(full, again)), "a second fill gives other bytes"
    cap = max(t - 3, 0)
    _, short = fill(cap)
    for a, b, g in zip(full, short, (I32_GUARD, I32_GUARD, U8_GUARD, U8_GUARD)):
        assert (b[:cap] == a[:cap]).all() and (b[cap:] == g).all(), "slots >= cap were written"
    ref, pos, strand, mm = full
    rows = [[(int(mm[i]), int(ref[i]), int(pos[i]), int(strand[i])) for i in range(off[r], off[r + 1])] for r in range(n)]
    return rows, counts


def check_world(w, reads, policies=POLICIES, modes=(True, False), m_values=(0,), raw=True):
    """Engine.list_valid_long over both parts == the model, per read and in order; the raw sweeps per part == the
    model's rows of that part as sets, the counts exact per stratum."""
    from mirge_amd.engine import STRATUM_ALL, STRATUM_BEST
    reads = list(reads) + [w.elem[c] for c in PLANTS[1:]] + [rnd(np.random.default_rng(99), 300)]
    cache = {}
    for name in policies:
        seed = MORE_POLICIES[name]
        hits = model_rows(w.world, reads, seed, cache)
        assert_not_hidden(reads, hits)
        for best in modes:
            for strands in (2, 1):
                for m in m_values:
                    off, entry, offset, strand, mm, supp = w.eng.list_valid_long(
                        reads, w.keys, strands=strands, stratum_mode=STRATUM_BEST if best else STRATUM_ALL, m=m, seed_len=seed[0],
                        max_mm_seed=seed[1], max_mm_total=seed[2])
                    assert len(off) == len(reads) + 1 and off[0] == 0 and len(supp) == len(reads)
                    for r, q in enumerate(reads):
                        want, want_supp = reported(hits[r], strands, best, m)
                        got = list(zip(mm[off[r]:off[r + 1]].tolist(), entry[off[r]:off[r + 1]].tolist(),
                                       offset[off[r]:off[r + 1]].tolist(), strand[off[r]:off[r + 1]].tolist()))
                        assert got == want, (name, best, strands, m, r, len(q), q[:40], got[:4], want[:4])
                        assert bool(supp[r]) == want_supp, (name, best, strands, m, r)
            if not raw:
                continue
            for p, key in enumerate(w.keys):
                lo, hi = w.world.base[p], w.world.base[p + 1]
                mute = [r for r in range(len(reads)) if r % 5 == 4]
                rows, counts = raw_listing(w.eng, w.eng.libs[key], reads, 2, seed, best, mute)
                for r in range(len(reads)):
                    mine = [h for h in hits[r] if lo <= h[1] < hi]
                    assert counts[:, r].tolist() == [sum(1 for h in mine if min(h[0], 3) == s) for s in range(4)], (name, p, r)
                    want = [] if r in mute else [(h[0], h[1] - lo, h[2], h[3]) for h in reported(mine, 2, best)[0]]
                    assert len(rows[r]) == len(set(rows[r])) and sorted(rows[r]) == sorted(want), (name, best, p, r, len(reads[r]))


LENGTHS = (256, 257, 287, 288, 289, 320, 511, 512, 513, 1000)


def test_lengths_at_the_word_edges(planted):
    """256 .. 1 000 nt on both strands with 0-2 substitutions, some of them to N: every policy, BEST and ALL."""
    w = planted
    reads = []
    for L in LENGTHS:
        for strand in (0, 1):
            for k in (0, 0, 1, 2):
                q = w.draw(L, strand)
                for i in w.rng.choice(L, size=k, replace=False):
                    q = sub(q, int(i), "N" if w.rng.random() < 0.15 else None)
                reads.append(q)
    check_world(w, reads)


@pytest.mark.parametrize("L", [1, 2, 15, 16, 31, 32, 33, 64, 65, 255])
def test_short_lengths_equal_the_packed_listing(planted, L):
    """The ragged form works for any length: the rows are exactly Engine.list_valid's on the same reads."""
    from mirge_amd import pack
    from mirge_amd.engine import ReadSet, STRATUM_ALL, STRATUM_BEST
    w = planted
    reads = [w.draw(L, s) for s in (0, 1) for _ in range(4)] + [w.elem[65][:L], revcomp(w.elem[130])[:L], w.rep[:L], rnd(w.rng, L)]
    reads += [sub(q, L // 2) for q in reads[:4]] + [sub(reads[0], 0, "N"), sub(reads[1], L - 1, "N")]
    words, lens, nmask = pack.pack_reads(reads)
    rs = ReadSet(words, lens, nmask, device=w.eng.device)
    listed = 0
    for seed in POLICIES.values():
        for mode in (STRATUM_BEST, STRATUM_ALL):
            how = dict(strands=2, stratum_mode=mode, m=3 if mode == STRATUM_ALL else 0, seed_len=seed[0], max_mm_seed=seed[1],
                       max_mm_total=seed[2])
            a = w.eng.list_valid(rs, w.keys, **how)
            b = w.eng.list_valid_long(reads, w.keys, **how)
            for x, y in zip(a, b):
                assert x.dtype == y.dtype and x.tolist() == y.tolist(), (L, seed, mode)
            listed += len(a[1])
    assert listed > 0 or L < 3


def rows_reads(w):
    reads = [w.elem[c] for c in PLANTS] + [revcomp(w.elem[65]), sub(w.elem[130], 200), sub(revcomp(w.elem[64]), 10)]
    return reads + [w.rep + w.rep_tail, revcomp(w.rep + w.rep_tail), sub(w.rep + w.rep_tail, 150), w.rep + rnd(w.rng, 276)]


@pytest.mark.parametrize("option", [None, ("wstop", 1), ("ftab", 0)])
def test_rows_per_interval(planted, option):
    """Elements with 0, 1, 63, 64, 65 and 130 copies, and a 24-nt repeat with 1 000 copies of which two continue as
    the read does: with the default options, with intervals searched down to one row, and without jump tables."""
    from mirge_amd.engine import DEFAULT_WSTOP
    w = planted
    if option:
        w.eng.set_option(*option)
    try:
        check_world(w, rows_reads(w))
    finally:
        w.eng.set_option("wstop", DEFAULT_WSTOP)
        w.eng.set_option("ftab", 1)


def test_first_piece_rule(planted):
    """Reads exact in every piece, and reads whose one or two seed mismatches lie in piece 0, in piece 1 and in the last
    piece, under K = 2 (-n 1, -v 1) and K = 3 (-v 2, and -n 2 -l 28): every alignment once, the counts exact."""
    w = planted
    reads = []
    for src in (w.elem[1], w.elem[65], revcomp(w.elem[130]), w.draw(300, 0), w.draw(300, 1)):
        reads.append(src)
        # -l 28 / -l 15 pieces (K = 2: [0,14) [14,28) and [0,7) [7,15); K = 3: [0,9) [9,18) [18,28)), -v halves and thirds
        for at in ((0,), (3,), (10,), (20,), (26,), (3, 20), (3, 10), (20, 26), (10, 16), (50,), (75,), (100,), (150,), (200,), (250,),
                   (299,), (50, 150), (150, 250), (120, 180), (250, 280), (50, 250)):
            q = src
            for i in at:
                q = sub(q, i)
            reads.append(q)
    check_world(w, reads, policies=["-n 1 -l 28", "-n 1 -l 15", "-n 2 -l 28", "-v 1", "-v 2"])


def test_seed_is_the_reads_5_prime_end_on_either_strand(planted):
    """-n 0 -l 25: a mismatch at read base 10 leaves the read unaligned whichever strand it comes from; the same
    mismatch at base 290 leaves it aligned with one mismatch.  Same planted locus, both orientations."""
    from mirge_amd.engine import STRATUM_ALL
    w = planted
    locus = w.elem[1]
    reads = [sub(locus, 10), sub(revcomp(locus), 10), sub(locus, 290), sub(revcomp(locus), 290)]
    off, entry, offset, strand, mm, supp = w.eng.list_valid_long(reads, w.keys, strands=2, stratum_mode=STRATUM_ALL, seed_len=25,
                                                                 max_mm_seed=0, max_mm_total=2)
    assert np.diff(off).tolist() == [0, 0, 1, 1]
    assert strand.tolist() == [0, 1] and mm.tolist() == [1, 1] and entry[0] == entry[1] and offset[0] == offset[1]
    check_world(w, reads, policies=["-n 0 -l 25", "-n 1 -l 28", "-v 1"])


def test_n_in_the_read_and_in_the_entries(planted):
    """An N of the read inside the seed, outside it (a mismatch), in every piece (nothing listed); an alignment that
    would cross an N run of the entry, and one that would cross into the next entry, whose bases the text holds right
    behind."""
    w = planted
    locus = w.elem[63]
    every_piece = locus
    for i in (2, 9, 16, 23, 120, 220):
        every_piece = sub(every_piece, i, "N")
    reads = [sub(locus, 5, "N"), sub(revcomp(locus), 5, "N"), sub(sub(locus, 5, "N"), 20, "N"), every_piece, revcomp(every_piece)]
    reads += [sub(s, i, "N") for s in (locus, revcomp(locus)) for i in (100, 150, 200, 250, 299)]     # outside the seed: a mismatch
    # an alignment that would cross an N run of the entry, and one that would cross into the next entry
    for p in range(2):
        s = w.entry(p, 3)
        at = s.index("N")
        lo = max(0, min(at - 100, len(s) - 300))
        reads += [s[lo:lo + 300].replace("N", "A"), revcomp(s[lo:lo + 300].replace("N", "C"))]
        a, b = w.entry(p, 0), w.entry(p, 1)
        reads += [a[-150:] + b[:150], revcomp(a[-150:] + b[:150]), a[-299:] + b[:1], a[-300:]]
    check_world(w, reads, policies=["-n 0 -l 28", "-n 0 -l 25", "-n 1 -l 28", "-n 1 -l 15", "-v 2"])


def test_edges(planted):
    """A read equal to a whole entry, a read one base longer than the longest entry, empty reads among others, and
    an empty batch."""
    from mirge_amd.engine import STRATUM_ALL
    w = planted
    whole = w.entry(0, 1)
    assert "N" not in whole and len(whole) > 255
    reads = [whole, revcomp(whole), "", whole + "C", "", "A" + whole]
    reads.append(max((s for _, ss in w.parts for s in ss), key=len).replace("N", "A") + "A")
    assert len(reads[-1]) == w.longest + 1
    check_world(w, reads, policies=["-n 0 -l 28", "-n 1 -l 15", "-v 2"])
    got = w.eng.list_valid_long([], w.keys, strands=2, stratum_mode=STRATUM_ALL)
    assert got[0].tolist() == [0] and all(len(x) == 0 for x in got[1:])
    rows, counts = raw_listing(w.eng, w.eng.libs[w.keys[0]], [], 2, (28, 0, 2), True)
    assert rows == [] and counts.shape == (4, 0)


def test_m_is_decided_over_all_parts(planted):
    """-m against the counts summed over the parts: the 65- and 130-copy reads are suppressed under -m 64, the 64-copy
    read is not."""
    check_world(planted, rows_reads(planted), policies=["-n 0 -l 25", "-n 1 -l 28"], m_values=(3, 64), raw=False)


def test_refusals(planted):
    import torch
    w = planted
    lib, eng = w.eng._lib, w.eng
    buf = torch.zeros(64, dtype=torch.int64, device=eng.device)
    p, st = buf.data_ptr(), eng._stream_ptr()
    good = dict(ctx=eng._h, words=p, nmask=None, word_off=p, lens=p, n=1, lib=eng.libs[w.keys[0]], strands=2, seed_len=28,
                max_mm_seed=0, max_mm_total=2)
    tail_fill = dict(stratum_mode=1, best_mm=p, offsets=p, cap=1, ref=p, pos=p, strand=p, mm=p)

    def call(fn, **change):
        a = dict(good, **{k: v for k, v in change.items() if k in good})
        args = [a[k] for k in good]
        if fn == "mrg_list_valid_long_count":
            args += [change.get("counts", p), st]
        else:
            t = dict(tail_fill, **{k: v for k, v in change.items() if k in tail_fill})
            args += [t[k] for k in tail_fill] + [st]
        return getattr(lib, fn)(*args)

    both = [dict(ctx=None), dict(words=None), dict(word_off=None), dict(lens=None), dict(lib=-1), dict(lib=99), dict(strands=0),
            dict(strands=3), dict(max_mm_seed=-1), dict(max_mm_seed=3, max_mm_total=3), dict(max_mm_seed=2, max_mm_total=1),
            dict(max_mm_total=4), dict(seed_len=0), dict(n=2 ** 31 - 1)]
    cases = [("mrg_list_valid_long_count", c) for c in both + [dict(counts=None)]]
    cases += [("mrg_list_valid_long_fill", c) for c in both + [dict(stratum_mode=2), dict(stratum_mode=-1), dict(best_mm=None),
                                                               dict(offsets=None), dict(ref=None), dict(pos=None), dict(strand=None),
                                                               dict(mm=None)]]
    for fn, change in cases:
        assert call(fn, **change) != 0, (fn, change)
        assert fn in lib.mrg_last_error().decode(), (fn, change)
    torch.cuda.current_stream(eng.device).synchronize()
    assert int(buf.abs().sum()) == 0      # refused before any launch: nothing was written
    # n == 0 is no error and launches nothing, whatever the buffers
    assert call("mrg_list_valid_long_count", n=0, words=None, word_off=None, lens=None, counts=None) == 0
    assert call("mrg_list_valid_long_fill", n=0, words=None, word_off=None, lens=None, best_mm=None, offsets=None) == 0


# ----------------------------------------------------------------------------------------------------------- front end

def front_world(seed, n_parts):
    """random_world's parts (entries of 700-1500 nt) with a 300-nt element planted 4 times over the parts, and its FASTA
    of 16-35-nt reads interleaved with ~40 reads of 256-600 nt: some lower-case, some with N, one that falls to 255 nt
    after -5 1 -3 2, the 4-copy element on either strand."""
    parts, fasta = random_world(seed, n_parts=n_parts, entries=3, entry_len=(700, 1500), n_reads=110)
    rng = np.random.default_rng(seed + 1)
    elem = rnd(rng, 300)
    for k in range(4):
        names, seqs = parts[k % n_parts]
        e = (k // n_parts) % len(seqs)
        at = int(rng.integers(0, len(seqs[e])))
        seqs[e] = seqs[e][:at] + (elem if k % 2 == 0 else revcomp(elem)) + seqs[e][at:]
    allseq = [s for _, ss in parts for s in ss]
    long_reads = [elem, revcomp(elem), sub(elem, 270), rnd(rng, 400)]
    for r in range(38):
        L = 258 if r == 0 else int(rng.integers(256, 601))
        src = allseq[int(rng.integers(0, len(allseq)))]
        at = int(rng.integers(0, len(src) - L))
        q = src[at:at + L].replace("N", "A")
        for i in rng.choice(L, size=int(rng.choice([0, 0, 1, 2, 3])), replace=False):
            q = sub(q, int(i), "N" if rng.random() < 0.2 else None)
        if rng.random() < 0.5:
            q = revcomp(q)
        long_reads.append(q.lower() if r % 7 == 3 else q)
    short = fasta.split(">")[1:]
    out, k = [], 0
    for i, rec in enumerate(short):
        out.append(">" + rec)
        if i % 2 == 1 and k < len(long_reads):
            out.append(">long%d some words\n%s\n" % (k, long_reads[k]))
            k += 1
    assert k == len(long_reads)
    return parts, "".join(out)


@pytest.fixture(autouse=True)
def long_reads_admitted(monkeypatch):
    """The front end lists reads beyond 255 nt when MIRGE_AMD_LONG_READS=1 (its child processes inherit it)."""
    monkeypatch.setenv("MIRGE_AMD_LONG_READS", "1")


@pytest.fixture(scope="module", params=[2, 3], ids=["two_parts", "three_parts"])
def front(request, tmp_path_factory, native_lib, oracle_lib):
    from tests.test_gpu_bowtie import write_parts
    d = tmp_path_factory.mktemp("front%d" % request.param)
    parts, fasta = front_world(500 + request.param, request.param)
    write_parts(parts, str(d / "lib"))
    (d / "reads.fa").write_text(fasta)
    return d, parts, fasta


@pytest.mark.parametrize("shape", range(len(SHAPES)))
def test_front_end_equals_model_with_long_reads(front, shape):
    """Each of the reference's nine bowtie shapes, as a fresh process: stdout and stderr are the model's, byte for
    byte -- both formats, MD:Z and the mismatch descriptors of 600-nt rows, -m summed over the parts."""
    from tests.test_gpu_bowtie import shim_align
    d, parts, fasta = front
    argv = SHAPES[shape][0] + [str(d / "lib"), str(d / "reads.fa")]
    want_out, want_err = btm.run(argv, parts, fasta)
    names, seqs = btm.read_fasta(fasta)
    a = btm.parse(argv)
    trimmed = {n: len(s) - a["t5"] - a["t3"] for n, s in zip(names, seqs)}
    lines = [l.split("\t") for l in want_out.splitlines() if not l.startswith("@")]
    aligned_long = {l[0] for l in lines if trimmed[l[0]] > 255 and (not a["sam"] or l[1] != "4")}
    assert len(aligned_long) >= 8                       # (the model itself aligns long reads here)
    if a["t5"] == 1 and a["t3"] == 2:
        assert 255 in trimmed.values()
    if a["m"]:
        assert any(l[0] == "long0" and l[-1] == "XM:i:4" for l in lines)    # 4 copies under -m 3: suppressed
    out, err = shim_align(argv)
    assert out == want_out
    assert err == want_err


def test_long_read_is_aligned_not_refused(native_lib, oracle_lib, tmp_path):
    """A 280-nt read against a 400-nt entry: status 0 and the model's lines, where the front end stops without
    MIRGE_AMD_LONG_READS=1; a read trimmed to nothing stays unaligned."""
    from mirge_amd.index import FmIndex
    from tests.test_gpu_bowtie import shim_align
    parts = [(["a"], ["ACGT" * 100])]
    FmIndex.build(*parts[0]).save(str(tmp_path / "x.mrgfm"))
    fasta = ">r\n" + "ACGT" * 70 + "\n>empty_after_trim\nAC\n"
    (tmp_path / "r.fa").write_text(fasta)
    for flags in (["-f", "-n", "0"], ["-f", "-v", "1", "-a", "-3", "2"]):
        argv = flags + [str(tmp_path / "x"), str(tmp_path / "r.fa")]
        out, err = shim_align(argv)
        want_out, want_err = btm.run(argv, parts, fasta)
        assert out == want_out and err == want_err
        assert out.startswith("r\t")
