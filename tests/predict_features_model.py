"""TEST INFRASTRUCTURE: predict mode's cluster feature table (reference miRge2.0.py:604, utils/generate_featureFiles.py and
classes/readCluster.py) in plain Python over lists and strings.  The one thing taken from the package is the pairwise
alignment, mirge_amd.a2i.local_pair: the first alignment `pairwise2.align.localms(cluster, read, 2, -1, -20, -20)` lists,
which tests/golden/a2i.json pins; `align=` swaps it.

    groups      parse: the consecutive table lines with one cluster name are one group, per chromosome, sorted as lists
    filter      passes: count sum >= 10, members >= 3, start > 20, end < chrLen - 20
    frame       frame: every member's padded row under the cluster's, H dashes before the cluster and T behind it
    columns     locate: count-weighted A/T/C/G per column, the majority base (ties: T, G, C, A), head / tail = the first /
                last column whose majority holds 5 c >= 4 total (float(c) / total >= 0.8 below 2^50)
    neighbours  neighbor: distances between the intervals (start + head - H, end + 1 + tail + T) and Good / Null / Bad
    nine        nine_columns: the re-padded frame, the genome template and the 3 + 6 feature columns
    text        run: `_features.tsv` and `_cluster.txt`

Stated deviations from the reference: a template range that leaves the chromosome is a ValueError (the reference slices a
shorter template and dies later or prints garbage); a template base other than A/C/G/T in the FIRST feature column writes
four `0` (the reference dies with UnboundLocalError; in a later column it repeats the previous column's four values, and so
does this); a base name beginning `mapped_mirna_` is a ValueError (the reference writes four more files there).
"""
import os

READ_COUNT_LIMIT, SEQ_COUNT_LIMIT, STABLE_LIMIT = 10, 3, 16 - 6 - 3
CLOSEST, FARTHEST, TERMINAL = 9, 44, 20
HEAD_SHIFT, TAIL_SHIFT = 3, 6
HEADER_HEAD = ("realMicRNA\trealMicRNAName\tchr\tstartPos\tendPos\tclusterName\tclusterSeq\tmajoritySeq\tstableClusterSeq\t"
               "alignedClusterSeq\tadjustedClusterSeq\tclusterSecondSeq\ttemplateSeq\tseqCount\treadCountSum\texactMatchRatio\t"
               "headUnstableLength\ttailUnstableLength\t")
FEATURES_SUFFIX, CLUSTER_SUFFIX = "_features.tsv", "_cluster.txt"
BASES = "ATCG"            # the reference's column order


def column_names():
    out = []
    for i in range(HEAD_SHIFT + TAIL_SHIFT):
        label = "head_minus%d_" % (HEAD_SHIFT - i) if i < HEAD_SHIFT else "tail_plus%d_" % (i + 1 - HEAD_SHIFT)
        out += [label + w for w in ("templateNucleotide", "TemplateNucleotide_percentage", "nonTemplateNucleotide_percentage",
                                    "A_percentage", "T_percentage", "C_percentage", "G_percentage")]
    return out


HEADER_TAIL = "\t".join(column_names()) + "\tneighborState\tupstreamDistance\tdownstreamDistance\n"


def py2_str(x):
    """str(x) as Python 2.7 prints it: a float as %.12g, `.0` appended when that shows neither `.` nor `e`."""
    if isinstance(x, float):
        s = "%.12g" % x
        return s if ("." in s or "e" in s or "n" in s) else s + ".0"
    return str(x)


def ratio_reached(c, total):
    """float(c) / total >= 0.8, decided in integers."""
    return 5 * c >= 4 * total


def name_fields(cname):
    """(chromosome, start, end, strand) of `<sample>:miRCluster_<i>_<len>:<chr>:<start>_<end><strand>`."""
    f = cname.split(":")
    a, b = f[-1][:-1].split("_")[:2]
    return f[2].strip(), int(a.strip()), int(b.strip()), cname[-1]


def parse(text):
    """(chromosomes sorted, {chromosome: groups sorted}), a group = [start, end, cluster name, cluster sequence, read names,
    read sequences, counts].  Columns 1, 2, 3, 4 and 6 of the table are read."""
    chroms, groups = [], {}
    for line in text.splitlines():
        f = line.strip().split("\t")
        name, count, seq, cseq, cname = f[0], int(f[1]), f[2], f[3], f[5]
        ch, start, end, _ = name_fields(cname)
        if ch not in groups:
            chroms.append(ch)
            groups[ch] = [[start, end, cname, cseq, [name], [seq], [count]]]
        elif groups[ch][-1][2] == cname:
            g = groups[ch][-1]
            g[4].append(name)
            g[5].append(seq)
            g[6].append(count)
        else:
            groups[ch].append([start, end, cname, cseq, [name], [seq], [count]])
    chroms.sort()
    for ch in chroms:
        groups[ch].sort()
    return chroms, groups


def passes(group, chr_len):
    return sum(group[6]) >= READ_COUNT_LIMIT and len(group[5]) >= SEQ_COUNT_LIMIT and group[0] > TERMINAL and \
        group[1] < chr_len - TERMINAL


def _default_align():
    from mirge_amd.a2i import local_pair
    return local_pair


def identity(cpad, spad):
    return sum(1 for a, b in zip(cpad, spad) if a == b and a != "-")


def frame(cseq, seqs, counts, align=None):
    """(rows, exact): rows[0] = the cluster's padded row, rows[1 + i] = member i's; exact = the summed counts of the members
    whose identity is their length."""
    align = align or _default_align()
    rows, exact = [], 0
    for seq, count in zip(seqs, counts):
        cpad, spad = align(cseq, seq)
        if identity(cpad, spad) == len(seq):
            exact += count
        if not rows:
            rows = [cpad, spad]
        elif cpad == rows[0]:
            rows.append(spad)
        else:
            h1 = cpad.index(cseq)
            h2 = rows[0].index(cseq)
            dh, dt = h1 - h2, (len(cpad) - h1) - (len(rows[0]) - h2)
            if dh > 0 or dt > 0:
                rows = ["-" * max(dh, 0) + r + "-" * max(dt, 0) for r in rows]
            rows.append("-" * max(-dh, 0) + spad + "-" * max(-dt, 0))
    return rows, exact


def dashes(s):
    """(leading, trailing) dashes."""
    return len(s) - len(s.lstrip("-")), len(s) - len(s.rstrip("-"))


def tallies(rows, counts, col):
    """{base: summed count} of the members' letters in one column; anything but A/T/C/G under "-"."""
    t = dict.fromkeys(BASES + "-", 0)
    for row, count in zip(rows[1:], counts):
        ch = row[col]
        t[ch if ch in BASES else "-"] += count
    return t


def locate(rows, counts):
    """(cluster ratios, majority sequence, majority ratios, head, tail); head / tail None without a stable column."""
    total = sum(counts)
    cratio, major, mratio, stable = [], "", [], []
    for i, cl in enumerate(rows[0]):
        t = tallies(rows, counts, i)
        cratio.append(float(t[cl]) / total if cl in BASES else 0)
        best, letter = max((t[b], b) for b in BASES)
        mratio.append(float(best) / total)
        major += letter
        stable.append(ratio_reached(best, total))
    if not any(stable):
        return cratio, major, mratio, None, None
    head = stable.index(True)
    last = len(stable) - 1 - stable[::-1].index(True)
    return cratio, major, mratio, head, last - len(stable)


def interval(group, rows, head, tail):
    H, T = dashes(rows[0])
    return group[0] + head - H, group[1] + 1 + tail + T


def neighbor(t, ivs, strands):
    """(state, upstream distance or None, downstream distance or None) of group t of a chromosome."""
    n = len(ivs)
    if n < 2:
        return "Null", None, None
    up = ivs[t][0] - ivs[t - 1][1] - 1 if t > 0 else None
    down = ivs[t + 1][0] - ivs[t][1] - 1 if t < n - 1 else None
    good_up = up is not None and CLOSEST <= up <= FARTHEST and strands[t - 1] == strands[t]
    good_down = down is not None and CLOSEST <= down <= FARTHEST and strands[t + 1] == strands[t]
    if up is not None and down is not None:
        state = "Good" if (good_up or good_down) else "Null" if (up > FARTHEST and down > FARTHEST) else "Bad"
    else:
        d = down if up is None else up
        state = "Good" if (good_up or good_down) else "Null" if d > FARTHEST else "Bad"
    return state, up, down


def revcomp(s):
    return s.translate(str.maketrans("ACGT", "TGCA"))[::-1]


def feature_columns(n_cols, head, tail):
    """The nine feature columns as indices into the UN-padded frame of n_cols columns (an index < 0 or >= n_cols is a
    padding column, all dashes), plus the two paddings: (columns, head padding, tail padding)."""
    tail_add = -tail - 1
    pad_h, pad_t = max(0, HEAD_SHIFT - head), max(0, TAIL_SHIFT - tail_add)
    tp = tail if pad_t == 0 else -TAIL_SHIFT
    return [head - HEAD_SHIFT + k for k in range(HEAD_SHIFT)] + [n_cols + pad_t + tp + k for k in range(TAIL_SHIFT)], pad_h, pad_t


def nine_columns(group, rows, counts, head, tail, chrom_seq):
    """calculateFeature: (adjusted cluster row, first member's row, template, 63 values, 45 counts)."""
    cols, pad_h, pad_t = feature_columns(len(rows[0]), head, tail)
    padded = ["-" * pad_h + r + "-" * pad_t for r in rows]
    hd, td = dashes(padded[0])
    strand = group[2][-1]
    lo, hi = (group[0] - hd, group[1] + td) if strand == "+" else (group[0] - td, group[1] + hd)
    if lo < 1 or hi > len(chrom_seq):
        raise ValueError("the template of %s leaves its chromosome" % group[2])
    template = chrom_seq[lo - 1:hi].upper()
    if strand != "+":
        template = revcomp(template)
    values, numbers = [], []
    pct = [0, 0, 0, 0]
    for x in cols:
        x += pad_h
        tn = template[x]
        t = tallies(padded, counts, x)
        numbers += [t[b] for b in BASES] + [t["-"]]
        acgt = sum(t[b] for b in BASES)
        if acgt == 0:
            t_pct, n_pct, pct = 0, 0, [0, 0, 0, 0]
        elif tn in BASES:
            other = acgt - t[tn]
            t_pct, n_pct = float(t[tn]) / acgt, float(other) / acgt
            pct = [0 if (b == tn or other == 0) else float(t[b]) / other for b in BASES]
        else:
            t_pct, n_pct = 0.0, 0.0          # (pct: the previous column's)
        values += [tn, t_pct, n_pct] + pct
    return padded[0], padded[1], template, values, numbers


def file_flags(table_path):
    f = os.path.basename(table_path).split("_")
    if f[0] == "mapped" and len(f) > 1 and f[1] == "mirna":
        raise ValueError("a table named mapped_mirna_* is compared with the known miRNA coordinates: not built")
    return ("-1" if f[0] == "mapped" else "Null"), "Null"


def run(table_text, chromosomes, table_path="x.tsv", align=None):
    """(`_features.tsv` text, `_cluster.txt` text, groups): chromosomes = {name: sequence}; groups = one dict per group
    that passed the filter, in the order of the files (those without a stable column have head = None and are in no file)."""
    flag, mirna = file_flags(table_path)
    chroms, by_chr = parse(table_text)
    feats, clus, info = [HEADER_HEAD], [], []
    seen = sum(len(by_chr[ch]) for ch in chroms)
    for ch in chroms:
        kept = []
        for g in by_chr[ch]:
            if not passes(g, len(chromosomes[ch])):
                continue
            rows, exact = frame(g[3], g[5], g[6], align)
            cratio, major, mratio, head, tail = locate(rows, g[6])
            H, T = dashes(rows[0])
            d = dict(cluster=g[2], chr=ch, start=g[0], end=g[1], strand=g[2][-1], members=len(g[5]), total=sum(g[6]), exact=exact,
                     H=H, T=T, head=head, tail=tail, rows=rows, counts=list(g[6]), written=False)
            info.append(d)
            if head is not None:
                kept.append((g, rows, exact, cratio, major, mratio, head, tail, d))
        ivs = [interval(k[0], k[1], k[6], k[7]) for k in kept]
        strands = [k[0][2][-1] for k in kept]
        for t, (g, rows, exact, cratio, major, mratio, head, tail, d) in enumerate(kept):
            state, up, down = neighbor(t, ivs, strands)
            clus.append("Cluster Name: %s\n%s (%d - %d%s) cluster %d:\n" % (g[2], ch, g[0], g[1], g[2][-1], t))
            clus.append("%s: %s\n%s: %s\n%s\n" % (rows[0], "\t".join(py2_str(x) for x in cratio), major,
                                                  "\t".join(py2_str(x) for x in mratio), rows[0]))
            clus += ["%s\t%d\n" % (r, c) for r, c in zip(rows[1:], g[6])]
            adjusted, second, template, values, numbers = nine_columns(g, rows, g[6], head, tail, chromosomes[ch])
            if len(feats) == 1:
                feats.append(HEADER_TAIL)
            tail_add = -tail - 1
            d.update(t=t, state=state, up=up, down=down, nine=numbers, template=template)
            if len(adjusted) - head - tail_add < STABLE_LIMIT:
                continue
            d["written"] = True
            majority = max((c, r) for c, r in zip(g[6], rows[1:]))[1].replace("-", "")
            stable = (rows[0][head:] if tail == -1 else rows[0][head:tail + 1]).replace("-", "")
            fields = [flag, mirna, ch, str(g[0]), str(g[1]), g[2], g[3], majority, stable, rows[0], adjusted, second, template,
                      str(len(g[5])), str(sum(g[6])), py2_str(float(exact) / sum(g[6])), str(head), str(tail_add)]
            fields += [py2_str(v) for v in values] + [state, py2_str(up), py2_str(down)]
            feats.append("\t".join(fields) + "\n")
    return "".join(feats), "".join(clus), dict(seen=seen, passed=len(info), groups=info)
