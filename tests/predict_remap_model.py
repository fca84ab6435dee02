"""TEST INFRASTRUCTURE: predict mode's second mapping (reference miRge2.0.py:566-601) in plain Python over lists and
strings; nothing from mirge_amd is imported.

The reference builds a bowtie index over `*_clusters_trimmed_orig.fa`, runs

    pass 1   bowtie <ix> <reads> -f -n 0 -l <seedLength> -S -a --best --norc
    pass 2   bowtie <ix> <reads pass 1 left unaligned> -f -n 1 -l 15 -5 1 -3 3 -S -a --best --strata --norc

and pushes the SAM text through split_fasta_from_sam, combineSam, decorateSam, parse_refine_sam (utils/processSam.py) and
`sort -k6,6 -k1,1`.  Here the same in three steps over arrays:

    rows    merge(listing1, listing2, sel): one row (read, cluster, offset, mm, pass) per listed alignment, pass 1 first
    order   sort_rows: stable by (cluster key, read key), the keys of name_key -- the byte order of the names
    text    table: 17 fields per row; the rows of one read on one cluster in the byte order of their lines (sort's last resort)

The order is `sort`'s in the C locale, a choice: under another locale sort collates differently.
"""
TRIM5, TRIM3 = 1, 3          # pass 2's -5 / -3
PASS2_SEED = (15, 1)         # -l 15 -n 1
KEY_DIGITS = 10


def pass1_argv(seed_length):
    return ["-f", "-n", "0", "-l", str(int(seed_length)), "-S", "-a", "--best", "--norc"]


PASS2_ARGV = ["-f", "-n", "1", "-l", "15", "-5", "1", "-3", "3", "-S", "-a", "--best", "--strata", "--norc"]


def parse_fasta(text):
    """(names up to the first whitespace, sequences) of a FASTA text."""
    names, seqs = [], []
    for line in text.splitlines():
        line = line.strip()
        if not line:
            continue
        if line[0] == ">":
            names.append(line[1:].split()[0])
            seqs.append("")
        else:
            seqs[-1] += line
    return names, seqs


def read_number(name):
    """n of `mir<n>_<count>`."""
    return int(name[3:].split("_")[0])


def cluster_number(name):
    """i of `<sample>:miRCluster_<i>_<len>:...`."""
    return int(name.split(":miRCluster_")[1].split("_")[0])


def name_key(number):
    """The fixed-width key whose integer order is the byte order of `<digits>_` among distinct numbers: the decimal digits
    left-aligned at 4 bits each, padded with 15 (`_` sorts after every digit)."""
    digits = str(int(number))
    assert len(digits) <= KEY_DIGITS
    key = 0
    for k in range(KEY_DIGITS):
        key = (key << 4) | (int(digits[k]) if k < len(digits) else 15)
    return key


def trim(seq, t5=TRIM5, t3=TRIM3):
    """bowtie's -5 / -3: a read of t5 + t3 bases or fewer becomes empty."""
    return seq[t5:len(seq) - t3] if len(seq) > t5 + t3 else ""


def merge(listing1, listing2, sel):
    """listing = (offsets [n + 1], cluster, offset, mm): read r owns rows [offsets[r], offsets[r + 1]); listing2 runs over the
    reads sel.  Rows (read, cluster, offset, mm, pass) in listing order, pass 1 first.  ValueError on contradicting arrays."""
    rows = []
    for p, (off, cl, pos, mm), reads in ((0, listing1, None), (1, listing2, sel)):
        n = len(off) - 1
        if len(cl) == 0:
            continue
        if n < 1 or off[0] != 0 or off[n] != len(cl) or any(off[r] > off[r + 1] for r in range(n)):
            raise ValueError("offsets do not ascend from 0 to the rows")
        for r in range(n):
            for k in range(off[r], off[r + 1]):
                rows.append((r if reads is None else int(reads[r]), int(cl[k]), int(pos[k]), int(mm[k]), p))
    return rows


def sort_rows(rows, read_numbers, cluster_numbers):
    """Stable from listing order by (cluster key, read key): what the device leaves."""
    return sorted(rows, key=lambda w: (name_key(cluster_numbers[w[1]]), name_key(read_numbers[w[0]])))


def line(name, seq, cname, cseq, offset, mm, second):
    q = trim(seq) if second else seq
    ref = cseq[offset:offset + len(q)]
    assert len(ref) == len(q) > 0
    md, run = "", 0
    for x, y in zip(q, ref):
        if x == y:
            run += 1
        else:
            md += "%d%s" % (run, y)
            run = 0
    md += str(run)
    return "\t".join([name, name.split("_")[-1], seq, cseq, "0", cname, str(offset + 1), "255", "%dM" % len(q), "*", "0", "0", q,
                      "I" * len(q), "XA:i:%d" % mm, "MD:Z:" + md, "NM:i:%d" % mm]) + "\n"


def table(sorted_rows, names, seqs, cnames, cseqs):
    """The file's text from rows in sort_rows' order."""
    out, k = [], 0
    while k < len(sorted_rows):
        e = k + 1
        while e < len(sorted_rows) and sorted_rows[e][:2] == sorted_rows[k][:2]:
            e += 1
        run = [line(names[r], seqs[r], cnames[c], cseqs[c], o, mm, p).encode() for r, c, o, mm, p in sorted_rows[k:e]]
        out += sorted(run)
        k = e
    return b"".join(out).decode()


def cluster_arrays(clusters_text):
    """A `_clusters_trimmed_orig.fa` text as the retained arrays of the trim: (names, sequences, kept [K] = number - 1,
    kept_seq_off [K + 1], kept_orig bytes)."""
    cnames, cseqs = parse_fasta(clusters_text)
    off = [0]
    for s in cseqs:
        off.append(off[-1] + len(s))
    return cnames, cseqs, [cluster_number(n) - 1 for n in cnames], off, "".join(cseqs).encode()


def sam_alignments(sam_text):
    """[(read name, cluster name, offset, mm)] of the aligned (FLAG 0) lines of a SAM text, in file order."""
    out = []
    for ln in sam_text.splitlines():
        if not ln or ln[0] == "@":
            continue
        f = ln.split("\t")
        if f[1] == "0":
            mm = [int(x[5:]) for x in f[11:] if x.startswith("XA:i:")][0]
            out.append((f[0], f[2], int(f[3]) - 1, mm))
    return out


def unaligned_fasta(sam1_text, reads_text):
    """split_fasta_from_sam: the reads without an aligned line in pass 1, as FASTA text."""
    done = set(a[0] for a in sam_alignments(sam1_text))
    names, seqs = parse_fasta(reads_text)
    return "".join(">%s\n%s\n" % (n, s) for n, s in zip(names, seqs) if n not in done)


def rows_from_sam(sam1_text, sam2_text, names, cnames):
    """The rows of the two SAM texts in listing order: pass 1's aligned lines, then pass 2's."""
    ri = {n: i for i, n in enumerate(names)}
    ci = {n: i for i, n in enumerate(cnames)}
    rows = [(ri[r], ci[c], o, mm, 0) for r, c, o, mm in sam_alignments(sam1_text)]
    rows += [(ri[r], ci[c], o, mm, 1) for r, c, o, mm in sam_alignments(sam2_text)]
    return rows


def table_from_sam(sam1_text, sam2_text, reads_text, clusters_text):
    """The whole stage from the two SAM texts and the two FASTA texts: (text, sorted rows)."""
    names, seqs = parse_fasta(reads_text)
    cnames, cseqs = parse_fasta(clusters_text)
    rows = sort_rows(rows_from_sam(sam1_text, sam2_text, names, cnames), [read_number(n) for n in names],
                     [cluster_number(n) for n in cnames])
    return table(rows, names, seqs, cnames, cseqs), rows
