#!/usr/bin/env python3
"""A stand-in for `RNAfold --noPS --noLP` for the tests and the timing script: our own small deterministic folder, not a
model of RNA energies.  Reads a FASTA on stdin (one sequence line per record) and writes RNAfold-shaped records on stdout:
the name cut at RNAfold's 41 characters, the sequence, and the structure with an energy.

The structure is a Nussinov maximum-pairing fold (hairpin loops of 3 or more) over the admissible pairs: A-U and C-G whose
bases lie in a run of HELIX complementary pairs that could stack (i + t with k - t), so that a random sequence folds into
a handful of stems as a real fold does, not into one lone pair per stem.  The traceback is fixed: a base stays unpaired
where that loses no pair, otherwise it takes its nearest partner that keeps the maximum.  Being admissible does not make
the neighbours pair: lone pairs and multiloops occur, unlike under --noLP.  The energy is -0.7 per pair, printed as
`(%6.2f)`, so both of RNAfold's shapes occur: `( -2.10)` and `(-10.50)`.  Options are accepted and ignored.
"""
import sys

import numpy as np

PAIRS = {("A", "U"), ("U", "A"), ("C", "G"), ("G", "C")}
MIN_LOOP = 3
HELIX = 4
NAME_CUT = 41


def admissible(seq):
    """ok[i][k]: seq[i] and seq[k] are complementary, a hairpin loop fits between them, and the run of such pairs
    (i + t, k - t) through them is at least HELIX long."""
    n = len(seq)
    code = np.array(["ACGU".find(c) for c in seq])
    partner = np.array([3, 2, 1, 0, -2])[code]       # (a base that is none of the four pairs with nothing)
    can = np.zeros((n + 2, n + 2), dtype=bool)      # (shifted by one: a frame of False around the matrix)
    at = np.arange(n)
    can[1:n + 1, 1:n + 1] = (code[:, None] == partner[None, :]) & (at[None, :] - at[:, None] > MIN_LOOP)
    inward = np.zeros((n + 2, n + 2), dtype=np.int32)
    outward = np.zeros((n + 2, n + 2), dtype=np.int32)
    for i in range(n, 0, -1):                       # the run from (i, k) towards the loop: (i + 1, k - 1), ...
        inward[i, 1:] = np.where(can[i, 1:], 1 + inward[i + 1, :-1], 0)
    for i in range(1, n + 1):                       # and away from it: (i - 1, k + 1), ...
        outward[i, :-1] = np.where(can[i, :-1], 1 + outward[i - 1, 1:], 0)
    return (can & (inward + outward - 1 >= HELIX))[1:n + 1, 1:n + 1]


def fold(seq):
    n = len(seq)
    if n == 0:
        return "", 0
    # best[i][j] = the most pairs in seq[i..j] (inclusive); rows n and n + 1 and column -1 (stored last) are zero
    ok = admissible(seq)
    best = np.zeros((n + 2, n + 1), dtype=np.int32)
    for i in range(n - 2, -1, -1):
        row = best[i + 1, :n].copy()
        for k in range(i + MIN_LOOP + 1, n):
            if ok[i, k]:
                cand = 1 + best[i + 1, k - 1] + best[k + 1, k:n]
                cand[0] = 1 + best[i + 1, k - 1]          # j == k: nothing behind the partner
                np.maximum(row[k:], cand, out=row[k:])
        row[:i + 1] = 0
        best[i, :n] = row
        best[i, i] = 0
    out = ["."] * n
    todo = [(0, n - 1)]
    while todo:
        i, j = todo.pop()
        while i < j and best[i, j] == best[i + 1, j]:
            i += 1
        if i >= j:
            continue
        for k in range(i + MIN_LOOP + 1, j + 1):
            behind = best[k + 1, j] if k < j else 0
            if ok[i, k] and 1 + best[i + 1, k - 1] + behind == best[i, j]:
                out[i], out[k] = "(", ")"
                todo.append((k + 1, j))
                todo.append((i + 1, k - 1))
                break
    return "".join(out), int(best[0, n - 1])


def main():
    lines = sys.stdin.read().splitlines()
    out, memo = [], {}
    for i in range(0, len(lines), 2):
        name = lines[i]
        seq = lines[i + 1].strip() if i + 1 < len(lines) else ""
        if seq not in memo:
            memo[seq] = fold(seq.upper().replace("T", "U"))
        structure, pairs = memo[seq]
        out.append("%s\n%s\n%s (%6.2f)\n" % (name[:1 + NAME_CUT], seq, structure, -0.7 * pairs if pairs else 0.0))
    sys.stdout.write("".join(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
