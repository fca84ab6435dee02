"""TEST INFRASTRUCTURE: a sequential model of predict mode's location clustering, written from the rule of the
reference's utils/cluster_basedon_location.py and from nothing in mirge_amd.

    cluster_tsv(sam_text, threshold, sample) -> the text of <...>_sorted_clusters.tsv
    sort_sam(sam_text) -> the SAM text in the order of mirge_amd.predict's sorted SAM file

Input is SAM text in coordinate order.  A line counts if its RNAME contains "chr" and its FLAG is 0 or 16; each
chromosome has one list per strand, walked in file order.  An alignment [s, e], e = s + len(SEQ) - 1, joins the current
cluster [S, E] of its list iff S <= s <= E and E - s + 1 >= threshold, else it opens a new one; on joining its name is
appended, and if e > E the sequence grows by SEQ[E - s + 1:] and E = e.  Output: chromosomes in order of first
appearance, all + clusters before all - clusters, numbered from 1 over the file.
"""
HEADER = "miRClusterID\tChr\tStrand\tStart\tEnd\tSequence\tSequenceLenght\tCoutOfReads\tCountOfMembers\tMembers\n"


def sample_of(file_name):
    return "_".join(file_name.split("/")[-1].split("_")[:-3])


def cluster_tsv(sam_text, threshold, sample):
    order, lists = [], {}
    for line in sam_text.splitlines():
        if not line or line[0] == "@":
            continue
        f = line.split("\t")
        name, flag, chrom, s, seq = f[0], f[1], f[2], int(f[3]), f[9]
        if "chr" not in chrom:
            continue
        if chrom not in lists:
            order.append(chrom)
            lists[chrom] = ([], [])
        if flag not in ("0", "16"):
            continue
        cl = lists[chrom][flag == "16"]
        e = s + len(seq) - 1
        if cl:
            cur = cl[-1]
            if cur["S"] <= s <= cur["E"] and cur["E"] - s + 1 >= threshold:
                cur["members"].append(name)
                if e > cur["E"]:
                    cur["seq"] += seq[cur["E"] - s + 1:]
                    cur["E"] = e
                continue
        cl.append(dict(S=s, E=e, seq=seq, members=[name]))
    out, i = [HEADER], 1
    for chrom in order:
        for strand, cl in zip("+-", lists[chrom]):
            for c in cl:
                reads = sum(int(m.split("_")[1]) for m in c["members"])
                out.append("\t".join(["%s:miRCluster_%d_%d" % (sample, i, len(c["seq"])), chrom, strand, str(c["S"]), str(c["E"]),
                                      c["seq"], str(len(c["seq"])), str(reads), str(len(c["members"])),
                                      ",".join(c["members"])]) + "\n")
                i += 1
    return "".join(out)


def sort_sam(sam_text, header=None):
    """Aligned lines by (entry in @SQ order, position, + before -, input order), then the FLAG 4 lines in input order;
    the header becomes `@HD VN:1.0 SO:coordinate` and the @SQ lines."""
    sq, aligned, rest = [], [], []
    for n, line in enumerate(sam_text.splitlines(True)):
        if line.startswith("@SQ"):
            sq.append(line)
        if line[0] == "@":
            continue
        f = line.split("\t")
        if f[1] in ("0", "16"):
            aligned.append((f[2], int(f[3]), f[1] == "16", n, line))
        else:
            rest.append(line)
    rank = {l.split("\t")[1][3:]: i for i, l in enumerate(sq)}
    aligned.sort(key=lambda a: (rank[a[0]], a[1], a[2], a[3]))
    return "".join(["@HD\tVN:1.0\tSO:coordinate\n"] + sq + [a[4] for a in aligned] + rest)
