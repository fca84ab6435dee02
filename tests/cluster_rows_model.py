"""TEST INFRASTRUCTURE: predict mode's location clusters from ARRAYS, one row at a time in plain Python -- the model of
what mrg_cluster_keys / _sort / _scan / _bounds / _assemble / _sorted_rows leave behind.  Written from the rule in
include/mirge_amd.h ("Predict mode's location clusters") and from tests/predict_cluster_model.py, which
tests/test_cluster_rows_model.py ties it to; nothing here comes from the kernels, and there is no scan: every row is
compared with the cluster IN FRONT OF IT in its (entry, strand) list.

    cluster_rows(parts, reads, counts, entry_keep, n_entries, threshold) -> dict
    sorted_rows(parts, n_entries, order, entry_keep) -> (read, entry, offset, strand, mm) columns
    random_rows(rng, ...) -> the keyword arguments of cluster_rows, rows drawn in piles around loci

A part is a dict: offsets [n_reads + 1] (read r owns the part's rows offsets[r] .. offsets[r + 1]), ref / pos / strand /
mm [rows] (pos 0-based, strand 0 = +), entry_base (the row's entry = entry_base + ref).  The rows of all parts are numbered
on in the order given.  A row of an entry >= n_entries, or of one with entry_keep[entry] == 0, is masked: it gets the
entry number n_entries, sorts behind all others and enters no cluster.
"""
import numpy as np

CLUSTER_ORDER, SAM_ORDER = 0, 1
_COMP = str.maketrans("ACGTN", "TGCAN")


def revcomp(s):
    return s[::-1].translate(_COMP)


def flat_rows(parts, n_entries, entry_keep):
    """[(key entry, true entry, pos, strand, read, mm)] in row order; key entry = n_entries for a masked row."""
    rows = []
    for p in parts:
        off = [int(x) for x in p["offsets"]]
        mm = p.get("mm")
        for r in range(len(off) - 1):
            for k in range(off[r], off[r + 1]):
                e = int(p["entry_base"]) + (int(p["ref"][k]) & 0xFFFFFFFF)
                masked = e >= n_entries or (entry_keep is not None and not entry_keep[e])
                rows.append((n_entries if masked else e, e, int(p["pos"][k]), 1 if p["strand"][k] else 0, r,
                             int(mm[k]) if mm is not None else 0))
    return rows


def ordered(rows, order):
    if order == CLUSTER_ORDER:
        return sorted(rows, key=lambda x: (x[0], x[3], x[2]))     # (stable: ties stay in row order)
    return sorted(rows, key=lambda x: (x[0], x[2], x[3]))


def sorted_rows(parts, n_entries, order, entry_keep=None):
    """The rows in either order as columns (read, entry, offset, strand, mm); the entry column is the key's."""
    rows = ordered(flat_rows(parts, n_entries, entry_keep), order)
    return (np.array([x[4] for x in rows], np.uint32), np.array([x[0] for x in rows], np.uint32),
            np.array([x[2] for x in rows], np.int64), np.array([x[3] for x in rows], np.uint8),
            np.array([x[5] for x in rows], np.uint8))


def cluster_rows(parts, reads, counts, entry_keep, n_entries, threshold):
    """Everything the C API yields for these rows: rows_cluster / rows_sam (the sorted rows, the first under the mask and
    the second without it), n_rows, n_valid, n_clusters, member [n_valid], entry / strand / start / end [K], member_off /
    len / seq_off [K + 1], seq (bytes), sum (Python ints).  reads: ACGTN strings; counts: one integer per read."""
    rows = ordered(flat_rows(parts, n_entries, entry_keep), CLUSTER_ORDER)
    valid = [x for x in rows if x[0] < n_entries]
    clusters, cur, cur_list = [], None, None
    for i, (e, _, pos, strand, r, _) in enumerate(valid):
        seq = revcomp(reads[r]) if strand else reads[r]
        s = pos + 1
        end = s + len(seq) - 1
        if (e, strand) != cur_list:
            cur, cur_list = None, (e, strand)
        if cur is not None and cur["S"] <= s <= cur["E"] and cur["E"] - s + 1 >= threshold:
            cur["n"] += 1
            cur["sum"] += int(counts[r])
            if end > cur["E"]:
                cur["seq"] += seq[cur["E"] - s + 1:]
                cur["E"] = end
            continue
        cur = dict(entry=e, strand=strand, S=s, E=end, seq=seq, first=i, n=1, sum=int(counts[r]))
        clusters.append(cur)
    K = len(clusters)
    lens = [len(c["seq"]) for c in clusters] + [0]
    seq_off = [0]
    for n in lens[:-1]:
        seq_off.append(seq_off[-1] + n)
    return dict(
        rows_cluster=sorted_rows(parts, n_entries, CLUSTER_ORDER, entry_keep),
        rows_sam=sorted_rows(parts, n_entries, SAM_ORDER, None),
        n_rows=len(rows), n_valid=len(valid), n_clusters=K,
        member=np.array([x[4] for x in valid], np.uint32),
        entry=np.array([c["entry"] for c in clusters], np.uint32), strand=np.array([c["strand"] for c in clusters], np.uint8),
        start=np.array([c["S"] for c in clusters], np.uint32), end=np.array([c["E"] for c in clusters], np.uint32),
        member_off=np.array([c["first"] for c in clusters] + [len(valid)], np.uint32),
        len=np.array(lens, np.uint32),
        seq_off=np.array(seq_off, np.uint64),
        seq="".join(c["seq"] for c in clusters).encode(),
        sum=[c["sum"] for c in clusters])


# ------------------------------------------------------------------------------------------------------- inputs
def make_parts(rows, n_reads, entry_bases, n_entries):
    """rows: [(read, entry, pos, strand, mm)] in any order -> parts split at entry_bases (part k holds the entries
    entry_bases[k] .. entry_bases[k + 1]), each part's rows grouped by read, a read's rows in the order given."""
    bounds = list(entry_bases) + [max(n_entries, 1 + max([r[1] for r in rows], default=0))]
    parts = []
    for k, base in enumerate(entry_bases):
        mine = sorted((r for r in rows if base <= r[1] < bounds[k + 1]), key=lambda r: r[0])
        off = np.zeros(n_reads + 1, np.uint64)
        np.cumsum(np.bincount([r[0] for r in mine], minlength=n_reads), out=off[1:])
        parts.append(dict(offsets=off, ref=np.array([r[1] - base for r in mine], np.int32), pos=np.array([r[2] for r in mine], np.int32),
                          strand=np.array([r[3] for r in mine], np.uint8), mm=np.array([r[4] for r in mine], np.uint8),
                          entry_base=base))
    return parts


def random_reads(rng, n_reads, max_len, short_below=1, n_rate=0.1):
    """Random ACGT strings of 1..max_len nt -- lengths at and around the 32-base words over-represented, a fifth
    shorter than `short_below` -- some with an N or two."""
    edges = [L for L in (1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 254, 255) if L <= max_len]
    reads = []
    for _ in range(n_reads):
        u = rng.random()
        if u < 0.2 and short_below > 1:
            L = int(rng.integers(1, min(short_below, max_len + 1)))
        elif u < 0.4:
            L = int(rng.choice(edges))
        else:
            L = int(rng.integers(1, max_len + 1))
        s = ["ACGT"[c] for c in rng.integers(0, 4, L)]
        if rng.random() < n_rate:
            for q in rng.integers(0, L, 2):
                s[int(q)] = "N"
        reads.append("".join(s))
    return reads


def random_rows(rng, n_rows, threshold, max_len=60, n_reads=None, n_entries=5, n_parts=2, pile=(1, 12), masked=1, max_count=97):
    """The keyword arguments of cluster_rows for exactly n_rows rows, drawn in piles around loci.  Every row of a pile
    is placed against the pile's end so far, E: an exact duplicate of the row before, the same position from another
    read, a contained row, an abutting row (s = E + 1), an overlap of exactly t - 1, t or t + 1, a read shorter than t,
    or a row a few bases on.  `masked` of the n_entries entries have entry_keep 0 (none: entry_keep is None)."""
    t = int(threshold)
    n_reads = n_reads or max(4, min(n_rows, 2000) // 2)
    reads = random_reads(rng, n_reads, max_len, short_below=t)
    short = [r for r, s in enumerate(reads) if len(s) < t]
    counts = rng.integers(1, max_count + 1, n_reads).astype(np.uint32)
    rows = []
    while len(rows) < n_rows:
        e, strand = int(rng.integers(0, n_entries)), int(rng.integers(0, 2))
        r = int(rng.integers(0, n_reads))
        pos = int(rng.integers(0, max(3000, 8 * n_rows)))   # (some piles run into each other)
        rows.append((r, e, pos, strand))
        S, E = pos + 1, pos + len(reads[r])
        for _ in range(int(rng.integers(pile[0], pile[1] + 1)) - 1):
            kind = int(rng.integers(0, 10))
            r = int(rng.integers(0, n_reads))
            if kind == 0:                                   # exact duplicate
                rows.append(rows[-1])
                continue
            if kind == 1:                                   # the same position, another read
                pos = rows[-1][2]
            elif kind == 2:                                 # contained, where the read fits
                pos = int(rng.integers(S - 1, max(S, E - len(reads[r]) + 1)))
            elif kind == 3:                                 # abutting: s = E + 1
                pos = E
            elif kind in (4, 5, 6):                         # overlap of exactly t - 1, t, t + 1
                pos = E - (t + kind - 5)
            elif kind == 7 and short:                       # shorter than the threshold, inside or at the end
                r = short[int(rng.integers(0, len(short)))]
                pos = int(rng.integers(max(S - 1, E - t - 2), E + 1))
            else:
                pos = E - int(rng.integers(0, 2 * t + 4))
            pos = max(pos, 0)
            rows.append((r, e, pos, strand))
            S, E = min(S, pos + 1), max(E, pos + len(reads[r]))
    rows = [r + (int(rng.integers(0, 3)),) for r in rows[:n_rows]]
    order = rng.permutation(n_rows)                         # (a read's rows in no particular order)
    rows = [rows[i] for i in order]
    n_parts = min(n_parts, n_entries)                       # (every part has an entry)
    bases = [0] + sorted(int(x) for x in rng.choice(np.arange(1, n_entries), n_parts - 1, replace=False))
    keep = None
    if masked:
        keep = np.ones(n_entries, np.uint8)
        keep[rng.choice(n_entries, masked, replace=False)] = 0
    return dict(parts=make_parts(rows, n_reads, bases, n_entries), reads=reads, counts=counts, entry_keep=keep,
                n_entries=n_entries, threshold=t)
