"""Predict mode's preliminary trim as plain sequential Python over arrays: the rule of the reference's preTrimClusteredSeq.py
and generate_Seq.py (miRge2.0.py:557-562) with this project's choice among repeat elements at equal distance -- the lower
element start first, then the lower index in the table sorted stably by start.  What mrg_predict_trim and
mrg_write_trimmed_clusters are compared with, and what the golden files of tests/golden/predict_trim.json pin.

The repeat table is flat: per entry (in the order of `entries`) a range rep_off[e] .. rep_off[e + 1] of (start, end, name id),
sorted stably by start, and the list of names.
"""
import bisect

HEADER_HEAD = "miRClusterID\tOriginalSeq\tFlag\trepetitiveElementName"
RUN = 6
_COMP = str.maketrans("ACGT", "TGCA")


def revcomp(s):
    return s[::-1].translate(_COMP)


def flat_repeats(entries, elements):
    """elements: {entry name: [(start, end, name), ...]} in any order -> (rep_off, start, end, name_id, names); entries the
    dict lacks get an empty range, names of the dict that are not entries are dropped."""
    rep_off, start, end, name_id, names, ids = [0], [], [], [], [], {}
    for e in entries:
        for s, t, nm in sorted(elements.get(e, []), key=lambda x: x[0]):   # (sorted() is stable)
            start.append(int(s))
            end.append(int(t))
            name_id.append(ids.setdefault(nm, len(ids)))
            if name_id[-1] == len(names):
                names.append(nm)
        rep_off.append(len(start))
    return rep_off, start, end, name_id, names


def nearest_two(start, lo, hi, at, high_first=False):
    """The (up to) two elements of start[lo:hi] (ascending) nearest `at`, nearer first.  At equal distance: the lower start,
    then the lower index (high_first: the opposite order, to find out what depends on the choice)."""
    p = bisect.bisect_left(start, at, lo, hi)
    cand = []
    if p > lo:                                   # the nearest lower start's run of equal starts, then the run before it
        a1 = bisect.bisect_left(start, start[p - 1], lo, p)
        cand += list(range(a1, p))
        if a1 > lo:
            cand += list(range(bisect.bisect_left(start, start[a1 - 1], lo, a1), a1))
    if p < hi:                                   # the same on the other side
        b1 = bisect.bisect_right(start, start[p], p, hi)
        cand += list(range(p, b1))
        if b1 < hi:
            cand += list(range(b1, bisect.bisect_right(start, start[b1], b1, hi)))
    sign = -1 if high_first else 1
    cand.sort(key=lambda i: (abs(start[i] - at), sign * start[i], sign * i))
    return cand[:2]


def nearest_two_brute(start, lo, hi, at, high_first=False):
    sign = -1 if high_first else 1
    return sorted(range(lo, hi), key=lambda i: (abs(start[i] - at), sign * start[i], sign * i))[:2]


def intersects(es, ee, cs, ce):
    return ee >= es and cs <= ce and es <= ce and ee >= cs


def trim(entry, strand, start, end, seq_off, seq, rep_off, rep_start, rep_end, cutoff, high_first=False):
    """-> dict(flag, rep, orig, kept, kept_seq_off, kept_orig); seq / orig / kept_orig are str."""
    flag, rep, orig = [], [], []
    for c in range(len(entry)):
        s = seq[seq_off[c]:seq_off[c + 1]]
        o = revcomp(s) if strand[c] else s
        orig.append(o)
        f, name = 0, -1
        if len(s) <= cutoff and not (len(o) >= RUN and (o[-RUN:] == "A" * RUN or o[:RUN] == "T" * RUN)):
            f = 1
            two = nearest_two(rep_start, rep_off[entry[c]], rep_off[entry[c] + 1], start[c], high_first)
            for x in reversed(two):              # (the nearer one last: its name stays)
                if intersects(rep_start[x], rep_end[x], start[c], end[c]):
                    f, name = 0, x
        flag.append(f)
        rep.append(name)
    kept = [c for c in range(len(entry)) if flag[c]]
    kept_seq_off = [0]
    for c in kept:
        kept_seq_off.append(kept_seq_off[-1] + len(orig[c]))
    return dict(flag=flag, rep=rep, orig="".join(orig), kept=kept, kept_seq_off=kept_seq_off,
                kept_orig="".join(orig[c] for c in kept))


def parse_table(text):
    """The cluster table's text -> (header fields, rows of fields)."""
    lines = text.split("\n")
    if lines and lines[-1] == "":
        lines.pop()
    return lines[0].split("\t"), [ln.split("\t") for ln in lines[1:]]


def table_arrays(rows, entries):
    """rows of parse_table -> the cluster arrays (entry numbers by `entries`)."""
    number = {e: i for i, e in enumerate(entries)}
    seq_off = [0]
    for r in rows:
        assert int(r[6]) == len(r[5])
        seq_off.append(seq_off[-1] + len(r[5]))
    return dict(entry=[number[r[1]] for r in rows], strand=[1 if r[2] == "-" else 0 for r in rows],
                start=[int(r[3]) for r in rows], end=[int(r[4]) for r in rows], seq_off=seq_off,
                seq="".join(r[5] for r in rows))


def files(table_text, elements, cutoff, high_first=False):
    """(trimmed.tsv, trimmed.fa, trimmed_orig.fa) as text from the cluster table's text and the elements per entry name."""
    entries = sorted({r[1] for r in parse_table(table_text)[1]})
    return files_flat(table_text, entries, flat_repeats(entries, elements), cutoff, high_first)


def files_flat(table_text, entries, flat, cutoff, high_first=False):
    """files() over a repeat table that is flat already (flat_repeats over `entries`): the loop alone."""
    head, rows = parse_table(table_text)
    a = table_arrays(rows, entries)
    rep_off, rs, re_, name_id, names = flat
    t = trim(a["entry"], a["strand"], a["start"], a["end"], a["seq_off"], a["seq"], rep_off, rs, re_, int(cutoff), high_first)
    tsv = ["\t".join([HEADER_HEAD] + head[1:]) + "\n"]
    fa, fo = [], []
    for c, r in enumerate(rows):
        o = t["orig"][a["seq_off"][c]:a["seq_off"][c + 1]]
        name = "*" if t["rep"][c] < 0 else names[name_id[t["rep"][c]]]
        tsv.append("\t".join([r[0], o, str(t["flag"][c]), name] + r[1:]) + "\n")
        if t["flag"][c]:
            where = ">%s:%s:%s_%s%s\n" % (r[0], r[1], r[3], r[4], r[2])
            fa.append(where + r[5] + "\n")
            fo.append(where + o + "\n")
    return "".join(tsv), "".join(fa), "".join(fo)


def outcomes(table_text, elements, cutoff, high_first=False):
    """Per row (flag, element name) -- what a tie order can change."""
    _, rows = parse_table(files(table_text, elements, cutoff, high_first)[0])
    return [(r[2], r[3]) for r in rows]


def member_arrays(rows):
    """rows of parse_table -> (read names, count_sum, member_off, members): the arrays the writers take, the names in the
    order of their first appearance."""
    names, number, count_sum, member_off, members = [], {}, [], [0], []
    for r in rows:
        count_sum.append(int(r[7]))
        for nm in r[9].split(","):
            if nm not in number:
                number[nm] = len(names)
                names.append(nm)
            members.append(number[nm])
        assert int(r[8]) == len(members) - member_off[-1]
        member_off.append(len(members))
    return names, count_sum, member_off, members


def world_inputs(table_text, elements):
    """What the array route needs of a golden world: (entries, rows, cluster arrays, read names, count_sum, member_off,
    members, the repeat file's text in the dict's own order).  Entries: the table's and the dict's chromosomes, sorted."""
    _, rows = parse_table(table_text)
    entries = sorted({r[1] for r in rows} | set(elements))
    names, count_sum, member_off, members = member_arrays(rows)
    tsv = "".join("%s\t%d\t%d\t%s\n" % (ch, e[0], e[1], e[2]) for ch, els in elements.items() for e in els)
    return entries, rows, table_arrays(rows, entries), names, count_sum, member_off, members, tsv
