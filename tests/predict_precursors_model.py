"""TEST INFRASTRUCTURE: predict mode's precursor candidates (reference miRge2.0.py:608, utils/get_precursors.py) in plain
Python over the text of `_features.tsv` and {chromosome: sequence}.

For every data line of the table, in file order:

    name    column `clusterName`; strand = its last character; chromosome = its third `:` field; start, end = the two
            numbers of its last `:` field
    H, T    the leading and trailing dashes of `alignedClusterSeq`; hu, tu = `headUnstableLength`, `tailUnstableLength`
    stable  on `+`  s = start - H + hu, e = end + T - tu;   on `-`  s = start - T + tu, e = end + H - hu
    windows precusor_1 = chr[max(0, s - 1 - 70) : e + 20], precusor_2 = chr[max(0, s - 1 - 20) : e + 70]: Python slices,
            the upper end clipped at the chromosome's length, an empty slice an empty line
    text    on `-` the slice is reverse-complemented; T -> U; `>name:precusor_1\\nSEQ\\n>name:precusor_2\\nSEQ\\n`

A name seen before is skipped (the reference asks `temp not in precusorList` of a list; a set here).  The rule cannot fire
on a table the feature stage wrote: every line is another cluster's and every cluster has its own name.  A chromosome the
dictionary does not hold is skipped, as the reference skips it.

Stated deviations from the reference:
  * bases come out as the index returns them (mrg_index_seq): upper case, N restored.  The reference would keep the lower
    case of a soft-masked genome.
  * a window whose upper end would be <= 0 is a ValueError (MRG_ERR_ARG in C): Python would count the negative end from
    the chromosome's far end.  The feature stage's filter (start > 20) rules it out, see DESIGN.md 8.14.
"""
UPSTREAM, DOWNSTREAM = 70, 20
SUFFIX = "_precusor.fa"
COMPLEMENT = str.maketrans("ACGTN", "TGCAN")


def dashes(aligned):
    """(H, T): the leading and trailing dashes of alignedClusterSeq."""
    return len(aligned) - len(aligned.lstrip("-")), len(aligned) - len(aligned.rstrip("-"))


def lines(features_text):
    """Per data line: (name, chromosome, strand, s, e), s .. e the stable part (1-based, inclusive)."""
    rows = features_text.split("\n")
    head = rows[0].strip().split("\t")
    col = {k: head.index(k) for k in ("headUnstableLength", "tailUnstableLength", "alignedClusterSeq")}
    out = []
    for line in rows[1:]:
        if line == "":
            break
        f = line.strip().split("\t")
        name = f[5]
        parts = name.split(":")
        start, end = (int(x.strip()) for x in parts[-1][:-1].split("_")[:2])
        H, T = dashes(f[col["alignedClusterSeq"]])
        hu, tu = int(f[col["headUnstableLength"]]), int(f[col["tailUnstableLength"]])
        if name[-1] == "+":
            s, e = start - H + hu, end + T - tu
        else:
            s, e = start - T + tu, end + H - hu
        out.append((name, parts[2], name[-1], s, e))
    return out


def windows(s, e, length):
    """[(lo, hi)] of precusor_1 and precusor_2: 0-based, half open, clipped to the chromosome as Python's slices clip."""
    out = []
    for up, down in ((UPSTREAM, DOWNSTREAM), (DOWNSTREAM, UPSTREAM)):
        lo, hi = max(0, s - 1 - up), e + down
        if hi <= 0:
            raise ValueError("a window ends at or before the chromosome's first base")
        hi = min(hi, length)
        out.append((min(lo, hi), hi))
    return out


def rna(dna, strand):
    dna = dna.upper()
    if strand == "-":
        dna = dna.translate(COMPLEMENT)[::-1]
    return dna.replace("T", "U")


def records(features_text, chroms):
    """[(name, strand, chromosome, lo, hi, sequence)], two per line written, in file order."""
    out, seen = [], set()
    for name, ch, strand, s, e in lines(features_text):
        if name in seen:
            continue
        if ch not in chroms:
            continue
        for lo, hi in windows(s, e, len(chroms[ch])):
            out.append((name, strand, ch, lo, hi, rna(chroms[ch][lo:hi], strand)))
        seen.add(name)
    return out


def run(features_text, chroms):
    """The text of `<table>_features_precusor.fa`."""
    return "".join(">%s:precusor_%d\n%s\n" % (r[0], 1 + (k & 1), r[5]) for k, r in enumerate(records(features_text, chroms)))
