"""The model of mrg_a2i_align (csrc/a2i_align.hip) in plain Python: the recurrence of DESIGN.md 8.6 cell by cell, with
gaps of any length, and the questions the -ai report asks of the ungapped frame.  It shares no code with
mirge_amd.a2i.local_pair / judge_align / a2i_editing, which it is tested against (tests/test_a2i_arrays.py); the
kernel is tested against it (tests/test_gpu_a2i_align.py)."""
import numpy as np

SIMPLE, ENDS, GAPPED, NOSCORE, UNSUPPORTED = 0, 1, 2, 3, 4
NEG = -10 ** 6


def scores(target, read):
    """-> (m, ends, (r_end, c_end) of the last best cell, g): the ungapped local score and where it ends, and the best
    score of a path that ends in a pair and holds a gap.  +2 / -1, -20 per gap base; an N equals nothing."""
    la, lb = len(target), len(read)
    U = [[0] * (lb + 1) for _ in range(la + 1)]
    Hg = [[NEG] * (lb + 1) for _ in range(la + 1)]
    E = [[NEG] * (lb + 1) for _ in range(la + 1)]
    F = [[NEG] * (lb + 1) for _ in range(la + 1)]
    for r in range(1, la + 1):
        for c in range(1, lb + 1):
            s = 2 if (target[r - 1] == read[c - 1] and read[c - 1] in "ACGT") else -1
            U[r][c] = max(0, U[r - 1][c - 1] + s)
            E[r][c] = max(U[r][c - 1], Hg[r][c - 1], E[r][c - 1]) - 20
            F[r][c] = max(U[r - 1][c], Hg[r - 1][c], F[r - 1][c]) - 20
            Hg[r][c] = max(Hg[r - 1][c - 1], E[r - 1][c - 1], F[r - 1][c - 1]) + s
    cells = [(r, c) for r in range(1, la + 1) for c in range(1, lb + 1)]
    m = max(U[r][c] for r, c in cells)
    tops = [(r, c) for r, c in cells if U[r][c] == m]
    g = max(Hg[r][c] for r, c in cells)
    return m, len(tops), tops[-1], g


def align_pair(target, read, from_base="A", to_base="G"):
    """-> (status, d, m, verdict, substring, mask) as the kernel's record holds them; target None or "" = no target."""
    if not target or len(target) > 32 or target.strip("ACGT") or not read or len(read) > 32:
        return UNSUPPORTED, 0, 0, 0, 0, 0
    la, lb = len(target), len(read)
    m, ends, (r_end, c_end), g = scores(target, read)
    if m <= 0:
        return NOSCORE, 0, 0, 0, 0, 0
    if ends != 1:
        return ENDS, 0, m, 0, 0, 0
    if g >= m:
        return GAPPED, 0, m, 0, 0, 0
    d = r_end - c_end
    # the frame: target position x holds read base x - d
    head_t, tail_t = max(0, -d), max(0, d + lb - la)
    first = max(0, d)
    last = min(la + tail_t - 4 - head_t, d + lb - 1)      # judge_align's end1 (padded length, quirk and all) and end2
    mat = mism = 0
    for x in range(first, last + 1):
        if x < la and target[x] == read[x - d]:
            mat += 1
        else:
            mism += 1                                       # (a base against the target's trailing dash too)
    need = la - 4 - (1 if d == 1 else 0)
    verdict = int(d <= 1 and not (mism > 1 or mat < need))
    substring = int(d >= 0 and d + lb <= la and target[d:d + lb] == read)
    mask = 0
    for x in range(0, la - 5):
        if 0 <= x - d < lb and target[x] == from_base and read[x - d] == to_base:
            mask |= 1 << x
    return SIMPLE, d, m, verdict, substring, mask


def pack_record(fields, target_id):
    status, d, m, verdict, substring, mask = fields
    return [status | verdict << 8 | substring << 9 | m << 16, d, mask - (1 << 32) if mask >> 31 else mask, target_id]


def records(table, seqs, pass_id, ref_id, keep=None, from_base="A", to_base="G", canon_pass=0, isomir_pass=8):
    """(idx uint32 [k], rec int32 [k, 4]) as Engine.a2i_align returns them, for reads given as strings."""
    idx, rec = [], []
    for i, seq in enumerate(seqs):
        p = int(pass_id[i])
        if p not in (canon_pass, isomir_pass) or (keep is not None and not keep[i]):
            continue
        tab = table.by_pass[p]
        e = int(ref_id[i])
        t = int(tab[e]) if 0 <= e < len(tab) else -1
        target = table.seqs[t] if t >= 0 and table.lens[t] else None
        idx.append(i)
        rec.append(pack_record(align_pair(target, seq, from_base, to_base), t))
    return np.array(idx, dtype=np.uint32), np.array(rec, dtype=np.int32).reshape(len(rec), 4)


# ------------------------------------------------------------------ the worlds both test files use
TIE_CASES = [   # tests/test_a2i.py: test_local_pair_ties_follow_pairwise2_order and its neighbours
    ("TGAGGTAGTAGGTTGTATAGTT", "TGAGGTAGTAGGTTGTATAGTT"),
    ("TGAGGTAGTAGGTTGTATAGTT", "GAGGTAGTAGGTTGTATAGTTA"),
    ("TGAGGTAGTAGGTTGTATAGTT", "TTTGAGGTAGTAGGTTGTATAGTT"),
    ("TGAGGTAGTAGGTTGTATAGTT", "AGGTAGTAGGTTGTATAGTT"),
    ("TGAGGTAGTAGGTTGTATAGTT", "TGAGGTAGCCGGTTGTATAGTT"),
    ("GC" + "A" * 18 + "TG", "A" * 17),
    ("TG" + "AC" * 9 + "GT", "AC" * 8),
    ("TGCATCGGATCGTACCTGAAGT", "TGCATCGGATCTACCTGAAGT"),
    ("CAGTTCGAGCTATGGACTTCAAGC", "CAGTTCGAGCTAGGACTTCAAGC"),
]


def random_pairs(n=4000, seed=606):
    """Pairs drawn as tests/test_a2i.py::test_local_pair_equals_the_generators_pairwise2 draws them."""
    import random
    rnd = random.Random(seed)

    def rs(k, alpha):
        return "".join(rnd.choice(alpha) for _ in range(k))
    out = []
    for _ in range(n):
        alpha = rnd.choice(["ACGT", "AC", "A", "ACG", "AAAC"])
        t = rs(rnd.randint(16, 27), alpha)
        kind = rnd.random()
        if kind < 0.4:
            s = list(t[rnd.randint(0, 5):len(t) - rnd.randint(0, 4)])
            for _k in range(rnd.randint(0, 2)):
                s[rnd.randrange(len(s))] = rnd.choice("ACGT")
            s = "".join(s) + rs(rnd.randint(0, 3), "ACGT")
        elif kind < 0.7:
            k = rnd.randint(5, len(t) - 5)
            s = t[:k] + t[k + 1:]
        elif kind < 0.85:
            k = rnd.randint(5, len(t) - 5)
            s = t[:k] + rnd.choice("ACGT") + t[k:]
        else:
            s = rs(rnd.randint(16, 26), alpha)
        out.append((t, s))
    return out


def isomir_world(n_targets=150, reads_per_target=12, seed=2024):
    """An isomiR-like world: targets of 19-25 nt (one in ten low-complexity) inside 4-nt flanks; a read is the target
    with a 5' shift of +-2, a 3' shift of +-3, 0-2 substitutions, one read in ten with a deleted base, 0-2 added
    bases.  -> [(target, read)]."""
    import random
    rnd = random.Random(seed)
    out = []
    for _ in range(n_targets):
        alpha = rnd.choice(["AC", "AAG", "AT"]) if rnd.random() < 0.1 else "ACGT"
        L = rnd.randint(19, 25)
        pre = "".join(rnd.choice("ACGT") for _ in range(4)) + "".join(rnd.choice(alpha) for _ in range(L)) + \
            "".join(rnd.choice("ACGT") for _ in range(4))
        target = pre[4:4 + L]
        for _k in range(reads_per_target):
            a = 4 + rnd.randint(-2, 2)
            b = 4 + L + rnd.randint(-3, 3)
            s = list(pre[a:b])
            for _j in range(rnd.randint(0, 2)):
                s[rnd.randrange(len(s))] = rnd.choice("ACGT")
            if rnd.random() < 0.1:
                del s[rnd.randrange(3, len(s) - 3)]
            s = "".join(s) + "".join(rnd.choice("ACGT") for _ in range(rnd.randint(0, 2)))
            out.append((target, s))
    return out
