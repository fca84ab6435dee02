"""Predict mode's candidate reads, stated plainly over arrays (the contract of DESIGN.md 8.10; what the reference's
convert2Fasta makes of unmapped.csv).  Shares no code with mirge_amd/.

With the reads in array order, total = the sum of a read's sample counts:
  raw list       the unmapped reads with total >= 1, numbered 1, 2, .. in array order
  filtered list  the unmapped reads with min_len <= length <= max_len and total >= cutoff, numbered likewise
  files          unmapped_mirna.fa (filtered, totals), unmapped_mirna_raw.fa (raw, totals) and per sample k
                 unmapped_mirna_<stem>.fa (filtered rows with count_k >= cutoff, count_k) and
                 unmapped_mirna_<stem>_raw.fa (raw rows with count_k >= 1, count_k); the numbers are the global ones
"""
import numpy as np


def csv_text(samples, seqs, quant, spike_in=False):
    """unmapped.csv as columnar.write_read_tables writes it: every row has annotFlag 0 and empty annotation slots."""
    names = ["exact miRNA", "hairpin miRNA", "mature tRNA", "primary tRNA", "snoRNA", "rRNA", "ncrna others", "mRNA",
             "isomiR miRNA"] + (["spike-in"] if spike_in else [])
    out = ["uniqueSequence,annotFlag," + ",".join(names) + "," + ",".join(samples) + "\n"]
    for seq, q in zip(seqs, quant):
        out.append("%s,0,%s,%s\n" % (seq, ",".join([""] * len(names)), ",".join(str(int(x)) for x in q)))
    return "".join(out)


def from_csv(text, spike_in=False):
    """(samples, seqs, quant rows) of an unmapped.csv text."""
    start = 12 if spike_in else 11
    lines = text.split("\n")
    samples = lines[0].split(",")[start:]
    seqs, quant = [], []
    for line in lines[1:]:
        if line:
            f = line.split(",")
            assert f[1] == "0", line
            seqs.append(f[0])
            quant.append([int(x) for x in f[start:]])
    return samples, seqs, quant


def select(lens, unmapped, quant, min_len, max_len, cutoff):
    """(total, raw_no, sel_no, n_raw, n_sel): Python ints per read; a number is 0 outside its list."""
    total, raw_no, sel_no = [], [], []
    j = i = 0
    for L, um, q in zip(lens, unmapped, quant):
        t = sum(int(x) for x in q)
        total.append(t)
        raw = bool(um) and t >= 1
        sel = bool(um) and min_len <= int(L) <= max_len and t >= cutoff
        j += raw
        i += sel
        raw_no.append(j if raw else 0)
        sel_no.append(i if sel else 0)
    return total, raw_no, sel_no, j, i


def sample_rows(numbers, quant, s, threshold):
    """[(read, number, count in s)] of a list for one sample."""
    return [(u, no, int(quant[u][s])) for u, no in enumerate(numbers) if no and int(quant[u][s]) >= threshold]


def stem(sample):
    return sample.strip().split(".")[0]


def fasta(rows, seqs):
    return "".join(">mir%d_%d\n%s\n" % (no, c, seqs[u]) for u, no, c in rows)


def files(samples, seqs, quant, min_len=16, max_len=25, cutoff=2, unmapped=None):
    """{file name: text} of the 2 + 2 S files (two samples with one stem: the later one's text)."""
    um = [True] * len(seqs) if unmapped is None else unmapped
    total, raw_no, sel_no, _, _ = select([len(s) for s in seqs], um, quant, min_len, max_len, cutoff)
    out = {"unmapped_mirna.fa": fasta([(u, no, total[u]) for u, no in enumerate(sel_no) if no], seqs),
           "unmapped_mirna_raw.fa": fasta([(u, no, total[u]) for u, no in enumerate(raw_no) if no], seqs)}
    for k, name in enumerate(samples):
        out["unmapped_mirna_%s.fa" % stem(name)] = fasta(sample_rows(sel_no, quant, k, cutoff), seqs)
    for k, name in enumerate(samples):
        out["unmapped_mirna_%s_raw.fa" % stem(name)] = fasta(sample_rows(raw_no, quant, k, 1), seqs)
    return out


def random_reads(rng, n, lengths, p_n=0.0):
    """n distinct reads with lengths drawn from `lengths`."""
    seen, out = set(), []
    while len(out) < n:
        L = int(rng.choice(lengths))
        s = "".join("ACGTN"[c] for c in rng.choice(5, L, p=[(1 - p_n) / 4] * 4 + [p_n]))
        if s not in seen:
            seen.add(s)
            out.append(s)
    return out


def as_arrays(seqs, quant, S):
    """(lens uint8, quant uint32 [n, S]) for the device calls; the reads must be at most 255 nt."""
    lens = np.array([len(s) for s in seqs], dtype=np.uint8)
    return lens, np.array(quant, dtype=np.uint32).reshape(len(seqs), S)
