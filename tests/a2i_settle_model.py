"""The model of mrg_a2i_settle (csrc/a2i_align.hip) in plain Python: which of the pairs whose best ungapped score ends in
several cells (status 1 of tests/a2i_align_model.py) `pairwise2.align.localms` answers with a plain ungapped frame, and
which frame.  It shares no code with mirge_amd.a2i, which it is tested against (tests/test_a2i_settle.py); the kernel
is tested against it (tests/test_gpu_a2i_settle.py).

With m > 0 and every gapped path below m (g < m), every best alignment is ungapped.  pairwise2 lists the best-scoring
cells in row order, tries them from the last one down and drops a walk back that meets another best cell before its
score falls to 0.  Three things decide the cell ("ties"):

  * a best cell is *eligible* iff it is the first cell with U == m in the positive run of its diagonal;
  * pairwise2 passes the best score along the last row and the last column without a penalty, so every cell to the
    right of a best cell in the last row, and below one in the last column, is listed as a best cell too;
  * the listing stops (it does not skip) at the first listed cell whose upper-left neighbour is listed: such a cell X is
    always one of the passed-along ones, and no cell after X in row order is tried.

The answer is the last eligible cell before X."""
from tests.a2i_align_model import ENDS, SIMPLE, align_pair, pack_record, scores   # noqa: F401  (re-exported for the tests)

TIED = 5

COUNTEREXAMPLES = [   # eligibility alone answers 10, 2 and 16
    ("AACACCCCAAACAAAAACCCAAAAA", "ACAAACCACCCAACAC", 1),
    ("AAAAAAAAAAAACCCAACAACAAAA", "ACAAAAAAAACAAAAA", -4),
    ("CGCAAACCTAGTGGAAAATATGTCGTT", "GATAGATCCACGACGATGACAA", -1),
]


def ungapped(target, read):
    la, lb = len(target), len(read)
    U = [[0] * (lb + 1) for _ in range(la + 1)]
    for r in range(1, la + 1):
        for c in range(1, lb + 1):
            s = 2 if (target[r - 1] == read[c - 1] and read[c - 1] in "ACGT") else -1
            U[r][c] = max(0, U[r - 1][c - 1] + s)
    return U


def tied_cell(target, read, m):
    """(r, c), 1-based, of the cell whose diagonal pairwise2 lists first; the caller has checked 0 < m and g < m."""
    la, lb = len(target), len(read)
    U = ungapped(target, read)
    tops = {(r, c) for r in range(1, la + 1) for c in range(1, lb + 1) if U[r][c] == m}
    listed = set(tops)
    for (r, c) in tops:
        if r == la:
            listed.update((la, x) for x in range(c, lb + 1))
        if c == lb:
            listed.update((x, lb) for x in range(r, la + 1))
    stop = min((cell for cell in listed if (cell[0] - 1, cell[1] - 1) in listed), default=(la + 1, 0))
    answer = None
    for (r, c) in sorted(tops):
        if (r, c) > stop:
            break
        k, first = 1, True
        while U[r - k][c - k] > 0:          # up the diagonal until the run's start
            if U[r - k][c - k] == m:
                first = False
            k += 1
        if first:
            answer = (r, c)
    return answer


def frame_fields(target, read, d, from_base, to_base):
    """(verdict, substring, mask) of the ungapped frame d, as align_pair computes them for a simple pair."""
    la, lb = len(target), len(read)
    head_t, tail_t = max(0, -d), max(0, d + lb - la)
    first = max(0, d)
    last = min(la + tail_t - 4 - head_t, d + lb - 1)
    mat = mism = 0
    for x in range(first, last + 1):
        if x < la and target[x] == read[x - d]:
            mat += 1
        else:
            mism += 1
    need = la - 4 - (1 if d == 1 else 0)
    verdict = int(d <= 1 and not (mism > 1 or mat < need))
    substring = int(d >= 0 and d + lb <= la and target[d:d + lb] == read)
    mask = 0
    for x in range(0, la - 5):
        if 0 <= x - d < lb and target[x] == from_base and read[x - d] == to_base:
            mask |= 1 << x
    return verdict, substring, mask


def settle_pair(target, read, from_base="A", to_base="G"):
    """align_pair's fields, with status 1 replaced by (TIED, d, m, verdict, substring, mask) where the rule claims the pair."""
    fields = align_pair(target, read, from_base, to_base)
    if fields[0] != ENDS:
        return fields
    m, _, _, g = scores(target, read)
    if g >= m:
        return fields
    r, c = tied_cell(target, read, m)
    d = r - c
    return (TIED, d, m) + frame_fields(target, read, d, from_base, to_base)


def settle_records(table, seqs, idx, rec, from_base="A", to_base="G"):
    """rec (int32 [k, 4], rows of status 1 included) after mrg_a2i_settle -> (rec, examined, settled)."""
    out = rec.copy()
    examined = settled = 0
    for row in range(len(idx)):
        if int(rec[row, 0]) & 0xFF != ENDS:
            continue
        examined += 1
        t = int(rec[row, 3])
        fields = settle_pair(table.seqs[t], seqs[int(idx[row])], from_base, to_base)
        if fields[0] == TIED:
            settled += 1
            out[row] = pack_record(fields, t)
    return out, examined, settled
