"""The statement of `annotate -tcf` (<sample>.trim.collapse.fa) in plain Python, as the reference writes the file
(quantReads.py:36-44): the distinct reads of a sample with a count, sorted as (count, sequence) tuples, reversed; one
">seq<i>_<count>" line and one sequence line per read.  The yardstick of tests/test_collapsed_fa_native.py and
tests/test_gpu_collapsed_order.py: everything is compared for equality."""
import numpy as np


def rows(seqs, counts, extra=()):
    """[(count, sequence)] of one sample in file order.  extra: further (sequence, count) pairs (the reads beyond 255 nt)."""
    pairs = [(int(c), s) for s, c in zip(seqs, counts) if int(c) > 0] + [(int(c), s) for s, c in extra if int(c) > 0]
    return sorted(pairs, reverse=True)


def order(seqs, counts):
    """The indices of the reads with a count in file order (uint32); equal (count, sequence) pairs in either order."""
    keyed = sorted(((int(c), s, u) for u, (s, c) in enumerate(zip(seqs, counts)) if int(c) > 0), reverse=True)
    return np.array([u for _, _, u in keyed], dtype=np.uint32)


def text(seqs, counts, extra=()):
    """The bytes of the file."""
    return "".join(">seq%d_%d\n%s\n" % (k + 1, c, s) for k, (c, s) in enumerate(rows(seqs, counts, extra))).encode()


def string_rank(seqs):
    """rank[u] = the position of seqs[u] in ascending string order (distinct strings)."""
    rank = np.empty(len(seqs), dtype=np.uint32)
    rank[np.array(sorted(range(len(seqs)), key=lambda u: seqs[u]), dtype=np.int64)] = np.arange(len(seqs), dtype=np.uint32)
    return rank


def random_reads(rng, n, lo=16, hi=40, p_n=0.02):
    """n DISTINCT reads of lo..hi nt, some with N."""
    seen, out = set(), []
    while len(out) < n:
        m = n - len(out)
        lens = rng.integers(lo, hi + 1, m)
        codes = rng.choice(5, size=(m, hi), p=[(1 - p_n) / 4] * 4 + [p_n])
        for L, row in zip(lens, codes):
            s = "".join("ACGTN"[c] for c in row[:L])
            if s not in seen:
                seen.add(s)
                out.append(s)
    return out
