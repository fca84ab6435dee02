"""A-to-I editing tally for `-ai`.

Restates writeDataToCSV.py:1221-1615 and its helpers (:35-229 judgeAllign, removeDash,
refineName, checkSeqList, align2TargetSeq, A2IEditing; :344-351 is in report.py):

  1. group the reads claimed by pass 0 / pass 8 per (merged) miRNA          :1224-1249
  2. keep reads whose best genome hit (-n 1 -a -3 2, both strands) is unique :1251-1287
  3. per miRNA x sample with RPM >= 1: align reads to the canonical sequence, count
     A->G per position, binomial p (p_mismatch 0.001)                       :1293-1321, :145-229
  4. Benjamini-Hochberg style adjustment per sample                         :1353-1364
  5. a2IEditing.report.csv (filters: a significant sample; canonical RPM >= 1; not in the
     repetitive-element list; the edited sequence does not occur in the genome -n 0 -3 2),
     a2IEditing.report.newform.csv, a2IEditing.detail.txt                   :1373-1594

Two things are not the reference's own arithmetic:
  * `pairwise2.align.localms(target, seq, 2, -1, -20, -20)` (Biopython, absent from the
    image and from /root/reference): `local_pair` restates its local alignment with affine gaps
    and Biopython 1.70-1.76's traceback order (which alignment is listed first among equals);
    the golden fixture answers the reference's call with an independent restatement of the
    same published algorithm.  Unpinned against a real Biopython.
  * the two genome bowtie runs: answered by a `genome` object with
      unique_best(reads) -> set of reads whose best stratum (<= 1 seed mismatch, 3' 2 nt
                            trimmed, both strands) holds exactly one alignment
      exact_hit(reads)   -> set of reads that align with 0 seed mismatches (same trimming)
    (mirge_amd.a2i.EngineGenome on the GPU, an exhaustive scan in the oracle).
The mismatch-type table (mismatchCountAnalysis, :248-342) is computed by the reference
and then deleted (:1536-1537), so it is not produced here.

a_to_i_report is the model and the route of `--ai-host`; `annotate -ai` itself runs a_to_i_report_arrays
(below) on the records of Engine.a2i_align and produces the same bytes.
"""
import math
import os

from .report import py2_float_str

P_MISMATCH = 0.001   # W2C:146
TAIL_SHIFT = 5       # W2C:147: the last 5 nt of the miRNA are not scored
PERCENT_CUTOFF = 2.0  # W2C:567
# W2C:1541-1551: run accessions of the reference's own study are relabelled in the newform table
SAMPLE_LABELS = {"SRR837842": "Colon 1", "SRR837839": "Colon 2", "SRR5127219": "Colon cell",
                 "SRR1646473": "Colon cancer 1", "SRR1646493": "Colon cancer 2", "SRR1917324": "DKO1",
                 "SRR1917336": "DLD1", "SRR1917329": "DKS8", "SRR567638": "Placenta 2"}


# ------------------------------------------------------------------ alignment
def _local_scores(target, seq, match, mismatch, gap_open, gap_extend):
    """Smith-Waterman scores as pairwise2's local mode fills them: score[r][c] = best alignment
    ending with target[:r] / seq[:c] consumed (floored at 0), a gap of n costing
    open + (n - 1) * extend, EXCEPT in the last row and the last column, where a gap is free
    (end gaps are not penalised: the best score is passed along).  `stretched[r][c]` says that the
    cell's score can come from a gap of two or more."""
    la, lb = len(target), len(seq)
    score = [[0] * (lb + 1) for _ in range(la + 1)]
    stretched = [[False] * (lb + 1) for _ in range(la + 1)]
    down = [0] + [2 * gap_open + gap_extend * (c - 1) for c in range(1, lb + 1)]   # gap in seq, per column
    for r in range(1, la + 1):
        tr = target[r - 1]
        across = 2 * gap_open + gap_extend * (r - 1)                               # gap in target, this row
        row, above = score[r], score[r - 1]
        for c in range(1, lb + 1):
            pair = above[c - 1] + (match if tr == seq[c - 1] else mismatch)
            opened, longer = (row[c - 1], across) if r == la else (row[c - 1] + gap_open, across + gap_extend)
            across = opened if opened >= longer else longer
            opened_d, longer_d = (above[c], down[c]) if c == lb else (above[c] + gap_open, down[c] + gap_extend)
            down[c] = opened_d if opened_d >= longer_d else longer_d
            top = max(pair, across, down[c])
            row[c] = top if top > 0 else 0
            stretched[r][c] = (across == top and longer == across) or (down[c] == top and longer_d == down[c])
    return score, stretched


def local_pair(target, seq, match=2, mismatch=-1, gap_open=-20, gap_extend=-20):
    """The first alignment `pairwise2.align.localms(target, seq, 2, -1, -20, -20)` lists, as the
    two sequences padded with '-' (W2C:109-111 reads [0][0] and [0][1]).  Biopython's order
    (releases 1.70-1.76, the ones a Python-2.7 miRge2.0 runs with) decides between alignments of
    equal score, and this follows it: candidates are the best-scoring cells that end in a pair,
    tried from the LARGEST (target position, read position) down; from a cell the walk back
    prefers a gap in the target, then a pair, then a gap in the read, depth first; a walk that
    meets another best-scoring cell is a zero-score extension of that cell's alignment and is
    dropped, as is a gap in the read placed right behind a gap in the target.  With -20 per
    gap base almost every read lands on one ungapped diagonal; the rule shows on low-complexity
    miRNAs (several diagonals tie: the one ending furthest along the miRNA wins) and on merged
    families whose members differ by an indel (one gap beats the best ungapped run).
    tests/golden/a2i.json pins it against the generator's own restatement (make_golden.py:
    pairwise2_localms, no product code)."""
    la, lb = len(target), len(seq)
    if la == 0 or lb == 0:
        raise ValueError("local_pair: empty sequence")
    score, stretched = _local_scores(target, seq, match, mismatch, gap_open, gap_extend)
    best = max(max(row) for row in score)
    tops = [(r, c) for r in range(la + 1) for c in range(lb + 1) if score[r][c] == best]
    top_set = set(tops)

    def pairs_here(r, c):
        return score[r - 1][c - 1] + (match if target[r - 1] == seq[c - 1] else mismatch) == score[r][c]

    candidates = []
    for (r, c) in tops:
        if (r - 1, c - 1) in top_set:
            break
        if best > 0 and pairs_here(r, c):
            candidates.append((r, c))

    def walk(r, c, cols, read_gap_last, first):
        """cols: alignment columns collected back to front as (target char, read char)."""
        while True:
            if not first:
                if (r, c) in top_set:
                    return None
                if r == 0 or c == 0 or score[r][c] <= 0:
                    if c and read_gap_last:
                        return None
                    return cols, r, c
            here = score[r][c]
            if stretched[r][c] and not first:
                raise ValueError("local_pair: alignment through a gap of two or more (%r, %r)" % (target, seq))
            moves = []
            if not first and not read_gap_last and r < la and score[r][c - 1] + gap_open == here:
                moves.append((r, c - 1, ("-", seq[c - 1]), False))
            if pairs_here(r, c):
                moves.append((r - 1, c - 1, (target[r - 1], seq[c - 1]), False))
            if not first and c < lb and score[r - 1][c] + gap_open == here:
                moves.append((r - 1, c, (target[r - 1], "-"), True))
            if not moves:
                return None
            for (r2, c2, col, flag) in moves[:-1]:
                got = walk(r2, c2, cols + [col], flag, False)
                if got is not None:
                    return got
            r, c, col, read_gap_last = moves[-1]
            cols = cols + [col]
            first = False

    for (r, c) in reversed(candidates):
        got = walk(r, c, [], False, True)
        if got is None:
            continue
        cols, r0, c0 = got
        body_t = "".join(x for x, _ in reversed(cols))
        body_s = "".join(y for _, y in reversed(cols))
        head = max(r0, c0)
        tail = max(la - r, lb - c)
        tpad = "-" * (head - r0) + target[:r0] + body_t + target[r:] + "-" * (tail - (la - r))
        spad = "-" * (head - c0) + seq[:c0] + body_s + seq[c:] + "-" * (tail - (lb - c))
        return tpad, spad
    raise ValueError("local_pair: no local alignment of %r and %r" % (target, seq))


def dash_count(s):
    head = len(s) - len(s.lstrip("-"))
    tail = len(s) - len(s.rstrip("-")) if head < len(s) else 0
    return head, tail


def remove_dash(s):
    return s.strip("-")


def judge_align(target_pad, seq_pad):
    """judgeAllign (W2C:35-69): the read may start at most 1 nt after the miRNA, and over the
    miRNA minus its last 3 nt it may show at most 1 mismatch and must show enough matches."""
    mismatch_limit, head_shift, tail_shift = 1, 1, 3
    head_t, tail_t = dash_count(target_pad)
    head_s, tail_s = dash_count(seq_pad)
    len1 = len(target_pad) - head_t - tail_t
    match_limit = len1 - tail_shift - mismatch_limit
    end1 = len(target_pad) - head_t - 1 - tail_shift
    end2 = len(seq_pad) - tail_s - 1
    if head_s - head_t > head_shift:
        return False
    mism = mat = 0
    for pos in range(head_t, min(end1, end2) + 1):
        if seq_pad[pos] == "-":
            continue
        if target_pad[pos] != seq_pad[pos]:
            mism += 1
        else:
            mat += 1
    need = match_limit - head_shift if head_s - head_t == head_shift else match_limit
    return not (mism > mismatch_limit or mat < need)


def align_to_target(target, seqs):
    """align2TargetSeq (W2C:101-143): pad everything into one frame; returns
    ([target_pad, read_pad...], [judge state...])."""
    frame, states = [], []
    for seq in seqs:
        tpad, spad = local_pair(target, seq)
        states.append(judge_align(tpad, spad))
        if not frame:
            frame = [tpad, spad]
        elif tpad == frame[0]:
            frame.append(spad)
        else:
            h1 = tpad.index(target)
            t1 = len(tpad) - h1 - len(target)
            h2 = frame[0].index(target)
            t2 = len(frame[0]) - h2 - len(target)
            if h1 >= h2:
                frame = ["-" * (h1 - h2) + x for x in frame]
            else:
                spad = "-" * (h2 - h1) + spad
            if t1 >= t2:
                frame = [x + "-" * (t1 - t2) for x in frame]
            else:
                spad = spad + "-" * (t2 - t1)
            frame.append(spad)
    return frame, states


def binom_cdf(k, n, p):
    """P[X <= k], X ~ Binomial(n, p) (scipy.stats.binom.cdf, W2C:220)."""
    from scipy import stats
    return float(stats.binom.cdf(k, n, p))


def a2i_editing(target, seqs, counts, mir_name, detail, retained, start_base="A", end_base="G"):
    """A2IEditing (W2C:145-229)."""
    frame, states = align_to_target(target, seqs)
    tpad = frame[0]
    start = tpad.index(target)
    end = start + len(target) - 1
    head = dash_count(tpad)[0]
    canonical = count_true = seq_true = 0
    pos_count, positions, kept = {}, [], []
    for j, spad in enumerate(frame[1:]):
        if states[j] and remove_dash(spad) in retained:
            if seqs[j] in target:
                canonical += counts[j]
            kept.append(spad)
            seq_true += 1
            count_true += counts[j]
            for i in range(start, end + 1 - TAIL_SHIFT):
                if i < len(spad) and tpad[i] == start_base and spad[i] == end_base:
                    p = i + 1 - head
                    if p not in pos_count:
                        positions.append(p)
                        pos_count[p] = counts[j]
                    else:
                        pos_count[p] += counts[j]
    detail.write("Canonical_Seq of %s: %s\n" % (mir_name, target))
    detail.write("seqList size is: %d, %d\n" % (len(seqs), len(counts)))
    for k, spad in enumerate(frame[1:]):
        detail.write("\t".join([spad, str(counts[k]), str(states[k])]) + "\n")
    detail.write("****************\n")
    detail.write("retained seqList size is: %d\n" % seq_true)
    for k, spad in enumerate(frame[1:]):
        if states[k]:
            detail.write("\t".join([spad, str(counts[k]), str(states[k])]) + "\n")
    detail.write("****************\n")
    detail.write("retained sequences after filering are:\n")
    for k, spad in enumerate(frame[1:]):
        if states[k] and remove_dash(spad) in retained:
            detail.write("\t".join([spad, str(counts[k]), str(states[k])]) + "\n")
    ratio, pval = {}, {}
    for p in positions:
        ratio[p] = float(pos_count[p]) / count_true if count_true else 0
        rest = count_true - pos_count[p]
        pval[p] = binom_cdf(rest, count_true, 1 - P_MISMATCH) if rest >= 0 else 1.0
    return kept, positions, pos_count, ratio, pval, count_true, seq_true, canonical


def refine_name(name):
    """refineName (W2C:75-86): drop the first '.fastq'."""
    at = name.find(".fastq")
    return name if at < 0 else name[:at] + name[at + len(".fastq"):]


def _check_seq_list(seq_pads, seqDic):
    """checkSeqList (W2C:88-99): is at least one kept read an exact (pass-0) miRNA read?"""
    for spad in seq_pads:
        rec = seqDic.get(remove_dash(spad))
        if rec is not None and rec["annot"][1] != "":
            return True
    return False


# ------------------------------------------------------------------ driver
def a_to_i_report(outputdir, sampleList, logDic, seqDic, mirDic, mirNameSeqDic, mirMergedNameDic,
                  removedMiRNAList, genome, start_base="A", end_base="G"):
    """The `if a_to_i:` block of writeDataToCSV (W2C:1221-1594).  Writes
    a2IEditing.detail.txt, a2IEditing.report.csv, a2IEditing.report.newform.csv and returns
    the rows of the final report (header included)."""
    S = len(sampleList)

    def rpm(count, i):
        return 1000000.0 * count / logDic["quantStats"][i]["mirnaReadsFiltered"]

    groups = {}
    for seq, rec in seqDic.items():
        annot = rec["annot"]
        if annot[1] == "" and annot[9] == "":
            continue
        name = annot[1] if annot[1] != "" else annot[9]
        name = mirMergedNameDic.get(name, name)
        if annot[1] != "" or any(rpm(rec["quant"][i], i) >= 1 for i in range(S)):
            groups.setdefault(name, []).append(seq)

    retained = genome.unique_best([s for seqs in groups.values() for s in seqs])

    site_values, site_order = {}, []
    with open(os.path.join(outputdir, "a2IEditing.detail.txt"), "w") as detail:
        for name, seqs in groups.items():
            target = mirNameSeqDic[name]
            for i in range(S):
                if not rpm(mirDic[name]["quant"][i], i) >= 1:
                    continue
                sel = [s for s in seqs if rpm(seqDic[s]["quant"][i], i) >= 1 or
                       (seqDic[s]["annot"][1] != "" and seqDic[s]["quant"][i] > 0)]
                cnt = [seqDic[s]["quant"][i] for s in sel]
                if len(cnt) > 1 and min(cnt) > 0:
                    kept, positions, pos_count, ratio, pval, count_true, seq_true, canonical = \
                        a2i_editing(target, sel, cnt, name, detail, retained, start_base, end_base)
                    for p in positions:
                        site = "%s:%s" % (name, p)
                        if site not in site_values:
                            site_order.append(site)
                            site_values[site] = [[] for _ in range(S)]
                        site_values[site][i] = site_values[site][i] + [
                            kept, str(sum(cnt)), str(len([c for c in cnt if c > 0])), str(count_true),
                            str(seq_true), str(canonical), str(pos_count[p]), ratio[p], pval[p]]

    for i in range(S):  # W2C:1353-1364
        ranked = sorted([site_values[s][i][8], s] for s in site_order if len(site_values[s][i]) != 0)
        for rank, (p, site) in enumerate(ranked):
            site_values[site][i].append(p * len(ranked) / (rank + 1))

    header = "miRNA,A-to-I position in the miRNA,miRNA sequence"
    for s in sampleList:
        n = refine_name(s)
        header += "," + ",".join([n + ".readCount", n + ".readCount.canonical", n + ".RPM.canonical",
                                  n + ".readCount.mismatch", n + ".RPM.mismatch", n + ".AtoI.percentage",
                                  n + ".AtoI.adjusted.pValue"])
    rows = []
    for site in site_order:
        name, pos = site.split(":")[0].strip(), site.split(":")[1].strip()
        cells = [name, pos, mirNameSeqDic[name]]
        for i in range(S):
            v = site_values[site][i]
            if len(v) == 0:
                cells += ["NE"] * 7
                continue
            base = [v[3], v[5], "%.2f" % rpm(int(v[5]), i), v[6], "%.2f" % rpm(int(v[6]), i)]
            if _check_seq_list(v[0], seqDic):
                base.append("%.2f%%" % (v[7] * 100))
                base.append("%.2E" % v[9] if v[9] <= 0.05 else "NS")
            else:
                base += ["NE", "NE"]
            cells += base
        rows.append(cells)

    def is_float(x):
        try:
            float(x)
            return True
        except ValueError:
            return False
    # keep rows with a significant sample (W2C:1423-1442), sort by name then position (:1444)
    rows = [r for r in rows if any(is_float(r[9 + i * 7]) for i in range((len(r) - 9) // 7 + 1))]
    rows.sort(key=lambda r: (r[0], int(r[1])))

    edited = {}
    for r in rows:  # W2C:1450-1480
        pos = int(r[1])
        edited_seq = "".join(end_base if k == pos - 1 else ch for k, ch in enumerate(r[2]))
        canon_rpm = [float(r[5 + i * 7]) if is_float(r[5 + i * 7]) else 0 for i in range((len(r) - 9) // 7 + 1)]
        edited[(r[0], r[1])] = dict(seq=edited_seq, rpm_drop=not any(x >= 1 for x in canon_rpm),
                                    repeat_drop=r[0] in removedMiRNAList)
    in_genome = genome.exact_hit([e["seq"] for e in edited.values()])
    final = [r for r in rows if not (edited[(r[0], r[1])]["rpm_drop"] or edited[(r[0], r[1])]["repeat_drop"] or
                                     edited[(r[0], r[1])]["seq"] in in_genome)]
    with open(os.path.join(outputdir, "a2IEditing.report.csv"), "w") as out:
        out.write(header + "\n")
        for r in final:
            out.write(",".join(r) + "\n")

    # a2IEditing.report.newform.csv (W2C:1554-1605)
    samples = []
    for item in header.split(","):
        if ".AtoI.percentage" in item and item.split(".")[0] not in samples:
            samples.append(item.split(".")[0])
    kept_sites = []
    for r in final:
        site = ":".join(r[:2])
        cells = r[3:]
        per = []
        for k in range(0, len(cells), 7):
            item = cells[k:k + 7]
            per.append(("NA", "NA") if item[6] in ("NE", "NS") else
                       (item[5][:-1], py2_float_str(math.log(float(item[4]), 2))))
        if any(x[0] != "NA" and float(x[0]) >= PERCENT_CUTOFF for x in per):
            kept_sites.append((site, per))
    ranked = sorted(((sum(1 for x in per if x[0] != "NA"), site) for site, per in kept_sites), reverse=True)
    by_site = dict(kept_sites)
    with open(os.path.join(outputdir, "a2IEditing.report.newform.csv"), "w") as out:
        out.write("miRNA:position,sample,A-to-I percentage,log2RPM\n")
        for k, sample in enumerate(samples):
            for _, site in ranked:
                out.write(site + "," + SAMPLE_LABELS.get(sample, sample) + "," + ",".join(by_site[site][k]) + "\n")
    return [header.split(",")] + final


# ------------------------------------------------------------------ the report from the arrays
# Engine.a2i_align (mrg_a2i_align, csrc/a2i_align.hip) aligns every miRNA read to its target on the GPU and answers with one
# 16-byte record per read; a_to_i_report_arrays groups, counts and writes from those records.  The functions above are the
# model: whatever follows must produce their bytes.
REC_INTS = 4
REC_FLAGS, REC_DIAG, REC_MASK, REC_TARGET = 0, 1, 2, 3
ST_SIMPLE, ST_ENDS, ST_GAPPED, ST_NOSCORE, ST_UNSUPPORTED = 0, 1, 2, 3, 4
ST_TIED = 5   # a row of status 1 that mrg_a2i_settle settled (Engine.a2i_align(settle=True)): filled as a row of status 0
BASE_CODE = {"A": 0, "C": 1, "G": 2, "T": 3}


class TargetTable:
    """Per merged miRNA (target id, in order of first appearance over the library's entries) its name and canonical
    sequence, and per cascade pass the map entry -> target id.  lens[t] = 0: the target has no sequence in
    mirNameSeqDic, or one that the kernel does not take (beyond 32 nt, a character other than ACGT)."""

    def __init__(self, names, seqs, words, lens, by_pass):
        self.names, self.seqs, self.words, self.lens, self.by_pass = names, seqs, words, lens, by_pass


def target_table(npp, mirMergedNameDic, mirNameSeqDic, canon_pass=0, isomir_pass=8):
    """What a_to_i_report asks per read (annot name -> merged name -> canonical sequence), once per library entry."""
    import numpy as np
    from . import pack
    ids, names, by_pass = {}, [], {}
    for p in (canon_pass, isomir_pass):
        tab = np.full(len(npp[p]), -1, dtype=np.int32)
        for e, entry in enumerate(npp[p]):
            name = mirMergedNameDic.get(entry, entry)
            if name not in ids:
                ids[name] = len(names)
                names.append(name)
            tab[e] = ids[name]
        by_pass[p] = tab
    seqs = [mirNameSeqDic.get(name) for name in names]
    usable = [s if (s is not None and 1 <= len(s) <= 32 and not s.strip("ACGT")) else "" for s in seqs]
    words, lens, _ = pack.pack_reads(usable, 1) if usable else (np.zeros((1, 0), np.uint64), np.zeros(0, np.uint8), None)
    return TargetTable(names, seqs, np.ascontiguousarray(words[0]), lens, by_pass)


def keep_mask(quant, pass_id, logDic, canon_pass=0):
    """The reads a_to_i_report groups, among those of the two miRNA passes: every read of the exact pass, and a read of
    the isomiR pass with RPM >= 1 in some sample (W2C:1224-1249)."""
    import numpy as np
    quant = np.asarray(quant)
    den = np.array([q["mirnaReadsFiltered"] for q in logDic["quantStats"]], dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        ok = (1000000.0 * quant.reshape(len(quant), -1) / den[None, :] >= 1).any(axis=1)
    return ok | (np.asarray(pass_id) == canon_pass)


def _genome_mask(genome, which, words, lens, nmask):
    """genome.<which> over packed reads as a boolean per read: its array form where it has one (EngineGenome), else
    the string form over the unpacked reads."""
    import numpy as np
    from . import pack
    form = getattr(genome, which + "_mask", None)
    if form is not None:
        return np.asarray(form(words, lens, nmask), dtype=bool)
    seqs = pack.unpack_reads(words, lens, nmask)
    hit = getattr(genome, which)(seqs)
    return np.fromiter((s in hit for s in seqs), dtype=bool, count=len(seqs))


def write_a2i_detail(path, words, lens, nmask, block_off, block_group, block_frame, block_text, group_names, group_targets,
                     row_read, row_count, row_flags, row_d):
    """a2IEditing.detail.txt through mrg_write_a2i_detail (csrc/a2i_detail_write.cpp); returns the lines written."""
    import ctypes as C
    import numpy as np
    from . import _native
    lib = _native.load()
    words = np.ascontiguousarray(words, dtype=np.uint64)
    W, n = words.shape
    lens = np.ascontiguousarray(lens, dtype=np.uint8)
    nm = None if nmask is None else np.ascontiguousarray(nmask, dtype=np.uint64)
    block_off = np.ascontiguousarray(block_off, dtype=np.uint64)
    nb = block_off.size - 1
    block_group = np.ascontiguousarray(block_group, dtype=np.int32)
    block_frame = np.ascontiguousarray(block_frame, dtype=np.int32).reshape(nb, 2)
    row_read = np.ascontiguousarray(row_read, dtype=np.uint32)
    row_count = np.ascontiguousarray(row_count, dtype=np.uint32)
    row_flags = np.ascontiguousarray(row_flags, dtype=np.uint8)
    row_d = np.ascontiguousarray(row_d, dtype=np.int32)
    texts = (C.c_char_p * max(nb, 1))(*[None if t is None else t.encode("ascii") for t in block_text])
    g_names = (C.c_char_p * max(len(group_names), 1))(*[x.encode("ascii") for x in group_names])
    g_targets = (C.c_char_p * max(len(group_targets), 1))(*[x.encode("ascii") for x in group_targets])
    lines = C.c_uint64(0)
    _native.check(lib.mrg_write_a2i_detail(
        os.fsencode(path), words.ctypes.data, W, n, lens.ctypes.data, None if nm is None else nm.ctypes.data, n, nb,
        block_off.ctypes.data, block_group.ctypes.data, block_frame.ctypes.data, texts, g_names, g_targets, len(group_names),
        row_read.ctypes.data, row_count.ctypes.data, row_flags.ctypes.data, row_d.ctypes.data, C.byref(lines)))
    return int(lines.value)


def a_to_i_report_arrays(outputdir, sampleList, logDic, words, lens, nmask, quant, pass_id, idx, rec, table, mirDic,
                         mirNameSeqDic, removedMiRNAList, genome, start_base="A", end_base="G", canon_pass=0, timings=None):
    """a_to_i_report from the host arrays of the run (words [W, n] / lens / nmask / quant [n, S] / pass_id) and the rows
    of Engine.a2i_align (idx [k], rec [k, 4], aligned with start_base / end_base) against `table` (target_table): the
    same three files, the same returned rows.  No Python loop runs over reads: the groups, the RPM selections, the
    frames and the counts are numpy over the records; Python walks the (miRNA, sample) blocks that hold an edited
    position, the sites, and -- through a2i_editing on strings unpacked for that block only -- the blocks whose
    selection holds a read the kernels did not settle (status other than 0 and 5).  Those blocks align only such reads, and each
    of them once, not once per sample: while they run, the module's local_pair is a memo of itself (it is a pure
    function of its arguments) that already holds the frames of the block's simple pairs.
    timings: a dict that receives `blocks`, `host_blocks`, `host_blocks_s`, `detail_write_s` and `tied_rows` (the rows of
    status 5 among those kept)."""
    global local_pair
    import io
    import time
    import numpy as np
    from . import pack
    S = len(sampleList)
    words = np.asarray(words, dtype=np.uint64)
    lens = np.asarray(lens, dtype=np.uint8)
    quant = np.asarray(quant).reshape(len(lens), -1)
    den_l = [q["mirnaReadsFiltered"] for q in logDic["quantStats"]]

    def rpm(count, i):
        return 1000000.0 * count / den_l[i]

    idx = np.asarray(idx).astype(np.int64)
    rec = np.asarray(rec, dtype=np.int32).reshape(-1, REC_INTS)
    keep = keep_mask(quant[idx], np.asarray(pass_id)[idx], logDic, canon_pass)
    idx, rec = idx[keep], rec[keep]
    k = int(idx.size)
    if k and any(d == 0 for d in den_l[:S]):
        raise ZeroDivisionError("float division by zero")   # (as rpm() of the record route)
    tid = rec[:, REC_TARGET].astype(np.int64)
    if k and (tid.min() < 0 or tid.max() >= len(table.names)):
        raise ValueError("a_to_i_report_arrays: a read without target id")
    canon = np.asarray(pass_id)[idx] == canon_pass
    q = quant[idx].astype(np.int64)                                      # [k, S]
    status = rec[:, REC_FLAGS] & 0xFF
    verdict = ((rec[:, REC_FLAGS] >> 8) & 1).astype(bool)
    substr = ((rec[:, REC_FLAGS] >> 9) & 1).astype(bool)
    settled = (status == ST_SIMPLE) | (status == ST_TIED)                # the record holds the frame
    diag = rec[:, REC_DIAG].astype(np.int64)
    mask = rec[:, REC_MASK].view(np.uint32)
    sub_w = np.ascontiguousarray(words[:, idx])
    sub_n = None if nmask is None else np.ascontiguousarray(np.asarray(nmask, dtype=np.uint64)[:, idx])
    retained = _genome_mask(genome, "unique_best", sub_w, lens[idx], sub_n) if k else np.zeros(0, dtype=bool)

    # groups in order of their first read
    uniq, first, gid = np.unique(tid, return_index=True, return_inverse=True)
    order = np.argsort(first, kind="stable")
    rank = np.empty(order.size, dtype=np.int64)
    rank[order] = np.arange(order.size)
    gid = rank[gid.reshape(-1)]
    g_tid = uniq[order]
    G = int(g_tid.size)
    g_names = [table.names[t] for t in g_tid]
    g_targets = [mirNameSeqDic[name] for name in g_names]               # (KeyError as the record route's)
    den = np.array(den_l[:S], dtype=np.float64)
    g_quant = np.array([mirDic[name]["quant"][:S] for name in g_names], dtype=np.float64).reshape(G, S)
    active = 1000000.0 * g_quant / den[None, :] >= 1 if G else np.zeros((0, S), dtype=bool)
    sel = ((1000000.0 * q / den[None, :] >= 1) | (canon[:, None] & (q > 0))) & active[gid] if k else np.zeros((0, S), bool)
    flat = gid[:, None] * S + np.arange(S)[None, :]                     # [k, S] -> block id
    n_sel = np.bincount(flat[sel], minlength=G * S)
    sel &= n_sel[flat] > 1                                                # (W2C:1309 len(cnt) > 1; every count is > 0)
    host = np.zeros(G * S, dtype=bool)
    host[flat[sel & ~settled[:, None]]] = True
    la = np.array([len(t) for t in g_targets], dtype=np.int64)[gid] if k else np.zeros(0, dtype=np.int64)
    lb = lens[idx].astype(np.int64)

    # per block, over its selected reads: the frame (align_to_target grows it to the largest head and tail pad) ...
    head = np.zeros(G * S, dtype=np.int64)
    tail = np.zeros(G * S, dtype=np.int64)
    pi, si = np.nonzero(sel)
    bi = flat[pi, si]
    np.maximum.at(head, bi, np.maximum(-diag[pi], 0))
    np.maximum.at(tail, bi, np.maximum(diag[pi] + lb[pi] - la[pi], 0))
    # ... and the counts over the reads judged True that the genome filter retained
    kept = sel & (verdict & retained)[:, None]
    kp, ks = np.nonzero(kept)
    kb = flat[kp, ks]
    kq = q[kp, ks]
    count_true = np.bincount(kb, weights=kq, minlength=G * S).astype(np.int64)
    seq_true = np.bincount(kb, minlength=G * S)
    canonical = np.bincount(kb, weights=kq * substr[kp], minlength=G * S).astype(np.int64)
    canon_kept = np.bincount(kb, weights=canon[kp], minlength=G * S) > 0
    sum_cnt = np.bincount(bi, weights=q[pi, si], minlength=G * S).astype(np.int64)
    pos_count, pos_first = {}, {}
    edited = mask[kp] != 0
    ep, eb, eq = kp[edited], kb[edited], kq[edited]
    em = mask[kp][edited]
    for b in range(32):
        has = (em >> np.uint32(b)) & np.uint32(1) != 0
        if not has.any():
            continue
        pos_count[b] = np.bincount(eb[has], weights=eq[has], minlength=G * S).astype(np.int64)
        f = np.full(G * S, k, dtype=np.int64)
        np.minimum.at(f, eb[has], ep[has])
        pos_first[b] = f

    # the rows of the detail file: (block, read) in block order, reads in array order
    by_block = np.argsort(bi, kind="stable")
    r_pi, r_si, r_bi = pi[by_block], si[by_block], bi[by_block]
    blocks = np.flatnonzero(n_sel > 1)
    blocks = blocks[np.bincount(bi, minlength=G * S)[blocks] > 0]
    block_off = np.zeros(blocks.size + 1, dtype=np.uint64)
    np.cumsum(np.bincount(bi, minlength=G * S)[blocks], out=block_off[1:].view(np.int64))
    block_text = [None] * int(blocks.size)

    site_values, site_order = {}, []

    def add_sites(name, i, positions, pos_cnt, values):
        for p in positions:
            site = "%s:%s" % (name, p)
            if site not in site_values:
                site_order.append(site)
                site_values[site] = [[] for _ in range(S)]
            c_true = values[2]
            ratio = float(pos_cnt[p]) / c_true if c_true else 0
            rest = c_true - pos_cnt[p]
            pval = binom_cdf(rest, c_true, 1 - P_MISMATCH) if rest >= 0 else 1.0
            site_values[site][i] = [values[0], str(values[1][0]), str(values[1][1]), str(c_true), str(values[3]),
                                    str(values[4]), str(pos_cnt[p]), ratio, pval]

    any_pos = np.zeros(G * S, dtype=bool)
    for b in pos_count:
        any_pos |= pos_count[b] > 0
    plain_pair, memo, host_s = local_pair, {}, 0.0

    def memo_pair(*args):
        if args not in memo:
            memo[args] = plain_pair(*args)
        return memo[args]
    for j, blk in enumerate(blocks.tolist()):
        g, i = divmod(blk, S)
        if host[blk]:   # a read the kernel did not settle: this block alone goes through the strings
            t_host = time.time()
            rows = r_pi[int(block_off[j]):int(block_off[j + 1])]
            seqs = pack.unpack_reads(np.ascontiguousarray(sub_w[:, rows]), lens[idx[rows]],
                                     None if sub_n is None else np.ascontiguousarray(sub_n[:, rows]))
            cnt = q[rows, i].tolist()
            text = io.StringIO()
            for seq, row in zip(seqs, rows.tolist()):   # what the kernel settled is not aligned again
                if settled[row] and (g_targets[g], seq) not in memo:
                    d_, la_, lb_ = int(diag[row]), len(g_targets[g]), len(seq)
                    memo[(g_targets[g], seq)] = ("-" * max(0, -d_) + g_targets[g] + "-" * max(0, d_ + lb_ - la_),
                                                 "-" * max(0, d_) + seq + "-" * max(0, la_ - d_ - lb_))
            local_pair = memo_pair
            try:
                kept_pads, positions, pos_cnt, _, _, c_true, s_true, canon_cnt = a2i_editing(
                    g_targets[g], seqs, cnt, g_names[g], text, {s for s, r in zip(seqs, retained[rows]) if r}, start_base,
                    end_base)
            finally:
                local_pair = plain_pair
            block_text[j] = text.getvalue()
            canon_seqs = {s for s, c in zip(seqs, canon[rows]) if c}
            add_sites(g_names[g], i, positions, pos_cnt,
                      (any(remove_dash(x) in canon_seqs for x in kept_pads), (sum(cnt), len(cnt)), c_true, s_true, canon_cnt))
            host_s += time.time() - t_host
        elif any_pos[blk]:
            found = sorted((int(pos_first[b][blk]), b) for b in pos_count if pos_count[b][blk] > 0)
            add_sites(g_names[g], i, [b + 1 for _, b in found], {b + 1: int(pos_count[b][blk]) for _, b in found},
                      (bool(canon_kept[blk]), (int(sum_cnt[blk]), int(n_sel[blk])), int(count_true[blk]),
                       int(seq_true[blk]), int(canonical[blk])))
    t_write = time.time()
    write_a2i_detail(os.path.join(outputdir, "a2IEditing.detail.txt"), words, lens, nmask, block_off, blocks // S,
                     np.stack([head[blocks], tail[blocks]], axis=1) if blocks.size else np.zeros((0, 2), np.int32),
                     block_text, g_names, g_targets, idx[r_pi], q[r_pi, r_si],
                     verdict[r_pi].astype(np.uint8) | (retained[r_pi].astype(np.uint8) << 1), diag[r_pi])
    if timings is not None:
        timings.update(blocks=int(blocks.size), host_blocks=int(host[blocks].sum()), host_blocks_s=host_s,
                       detail_write_s=time.time() - t_write, tied_rows=int((status == ST_TIED).sum()))
    return _write_reports(outputdir, sampleList, rpm, site_order, site_values, mirNameSeqDic, removedMiRNAList, genome,
                          end_base)


def _write_reports(outputdir, sampleList, rpm, site_order, site_values, mirNameSeqDic, removedMiRNAList, genome, end_base):
    """a_to_i_report from the Benjamini-Hochberg adjustment on (W2C:1353-1594), over per-site values whose first cell
    is checkSeqList's answer (a kept read is an exact miRNA read) and not the kept reads themselves."""
    S = len(sampleList)
    for i in range(S):  # W2C:1353-1364
        ranked = sorted([site_values[s][i][8], s] for s in site_order if len(site_values[s][i]) != 0)
        for rank, (p, site) in enumerate(ranked):
            site_values[site][i].append(p * len(ranked) / (rank + 1))

    header = "miRNA,A-to-I position in the miRNA,miRNA sequence"
    for s in sampleList:
        n = refine_name(s)
        header += "," + ",".join([n + ".readCount", n + ".readCount.canonical", n + ".RPM.canonical",
                                  n + ".readCount.mismatch", n + ".RPM.mismatch", n + ".AtoI.percentage",
                                  n + ".AtoI.adjusted.pValue"])
    rows = []
    for site in site_order:
        name, pos = site.split(":")[0].strip(), site.split(":")[1].strip()
        cells = [name, pos, mirNameSeqDic[name]]
        for i in range(S):
            v = site_values[site][i]
            if len(v) == 0:
                cells += ["NE"] * 7
                continue
            base = [v[3], v[5], "%.2f" % rpm(int(v[5]), i), v[6], "%.2f" % rpm(int(v[6]), i)]
            if v[0]:
                base.append("%.2f%%" % (v[7] * 100))
                base.append("%.2E" % v[9] if v[9] <= 0.05 else "NS")
            else:
                base += ["NE", "NE"]
            cells += base
        rows.append(cells)

    def is_float(x):
        try:
            float(x)
            return True
        except ValueError:
            return False
    rows = [r for r in rows if any(is_float(r[9 + i * 7]) for i in range((len(r) - 9) // 7 + 1))]
    rows.sort(key=lambda r: (r[0], int(r[1])))

    edited = {}
    for r in rows:  # W2C:1450-1480
        pos = int(r[1])
        edited_seq = "".join(end_base if k == pos - 1 else ch for k, ch in enumerate(r[2]))
        canon_rpm = [float(r[5 + i * 7]) if is_float(r[5 + i * 7]) else 0 for i in range((len(r) - 9) // 7 + 1)]
        edited[(r[0], r[1])] = dict(seq=edited_seq, rpm_drop=not any(x >= 1 for x in canon_rpm),
                                    repeat_drop=r[0] in removedMiRNAList)
    in_genome = genome.exact_hit([e["seq"] for e in edited.values()])
    final = [r for r in rows if not (edited[(r[0], r[1])]["rpm_drop"] or edited[(r[0], r[1])]["repeat_drop"] or
                                     edited[(r[0], r[1])]["seq"] in in_genome)]
    with open(os.path.join(outputdir, "a2IEditing.report.csv"), "w") as out:
        out.write(header + "\n")
        for r in final:
            out.write(",".join(r) + "\n")

    samples = []   # a2IEditing.report.newform.csv (W2C:1554-1605)
    for item in header.split(","):
        if ".AtoI.percentage" in item and item.split(".")[0] not in samples:
            samples.append(item.split(".")[0])
    kept_sites = []
    for r in final:
        site = ":".join(r[:2])
        cells = r[3:]
        per = []
        for k in range(0, len(cells), 7):
            item = cells[k:k + 7]
            per.append(("NA", "NA") if item[6] in ("NE", "NS") else
                       (item[5][:-1], py2_float_str(math.log(float(item[4]), 2))))
        if any(x[0] != "NA" and float(x[0]) >= PERCENT_CUTOFF for x in per):
            kept_sites.append((site, per))
    ranked = sorted(((sum(1 for x in per if x[0] != "NA"), site) for site, per in kept_sites), reverse=True)
    by_site = dict(kept_sites)
    with open(os.path.join(outputdir, "a2IEditing.report.newform.csv"), "w") as out:
        out.write("miRNA:position,sample,A-to-I percentage,log2RPM\n")
        for k, sample in enumerate(samples):
            for _, site in ranked:
                out.write(site + "," + SAMPLE_LABELS.get(sample, sample) + "," + ",".join(by_site[site][k]) + "\n")
    return [header.split(",")] + final


# ------------------------------------------------------------------ genome filters on the GPU
_COMP = {"A": "T", "C": "G", "G": "C", "T": "A", "N": "N"}


def revcomp(s):
    return "".join(_COMP.get(ch, "N") for ch in reversed(s))


class EngineGenome:
    """The two genome bowtie runs of the -ai path on the GPU engine: the genome (one or several
    libraries, e.g. one per chromosome) is searched with the reads and with their reverse
    complements (no --norc in W2C:1263/:1488), after dropping the last 2 nt (-3 2)."""

    def __init__(self, engine, library_keys):
        self.engine = engine
        self.keys = list(library_keys)

    def _best(self, reads, max_mm_seed):
        """-> (best_mm, count, undecided) over all parts and both strands.  undecided: some part answered
        (255, 255) for a strand -- a seed too repetitive to be walked and no alignment among the rows that were
        (include/mirge_amd.h: mrg_count_best); what that part holds for the read is not known."""
        import numpy as np
        from . import pack
        from .engine import ReadSet
        trimmed = [r[:-2] for r in reads]
        both = trimmed + [revcomp(r) for r in trimmed]
        n = len(reads)
        best_mm = np.full(n, 255, dtype=np.int32)
        count = np.zeros(n, dtype=np.int64)
        undecided = np.zeros(n, dtype=bool)
        if n == 0:
            return best_mm, count, undecided
        words, lens, nmask = pack.pack_reads(both)
        rs = ReadSet(words, lens, nmask, None, device=self.engine.device)
        for key in self.keys:
            mm, cnt = self.engine.count_best(rs, key, seed_len=28, max_mm_seed=max_mm_seed, max_mm_total=2)
            for half in (slice(0, n), slice(n, 2 * n)):
                m, c = mm[half].astype(np.int32), cnt[half].astype(np.int64)
                undecided |= (m == 255) & (c == 255)
                better = m < best_mm
                same = (m == best_mm) & (m < 255)
                count = np.where(better, c, np.where(same, count + c, count))
                best_mm = np.where(better, m, best_mm)
        return best_mm, count, undecided

    def unique_best(self, reads):
        """An undecided part makes the read non-unique: a sequence that repetitive there has no unique best hit."""
        reads = list(dict.fromkeys(reads))
        mm, cnt, und = self._best(reads, 1)
        return {r for r, m, c, u in zip(reads, mm, cnt, und) if m < 255 and c == 1 and not u}

    def exact_hit(self, reads):
        """An undecided part counts as a hit: the edited sequence is then taken to occur in the genome and its
        site leaves the report (W2C:1488-1496), the reading that never reports a site the genome explains."""
        reads = list(dict.fromkeys(reads))
        mm, _, und = self._best(reads, 0)
        return {r for r, m, u in zip(reads, mm, und) if m < 255 or u}

    # ---- the array forms: a boolean per read of a packed read set, nothing per read in Python
    def _best_packed(self, words, lens, nmask, max_mm_seed):
        """_best for packed reads: the `-3 2` trim and the reverse complement are done on the codes of each length
        class (numpy), the reads are never strings."""
        import numpy as np
        from . import pack
        from .engine import ReadSet
        words = np.asarray(words, dtype=np.uint64)
        lens = np.asarray(lens).astype(np.int64)
        n = int(lens.size)
        best_mm = np.full(n, 255, dtype=np.int32)
        count = np.zeros(n, dtype=np.int64)
        undecided = np.zeros(n, dtype=bool)
        if n == 0:
            return best_mm, count, undecided
        cut = np.maximum(lens - 2, 0)
        W = pack.words_for(max(int(cut.max()), 1))
        both_w = np.zeros((W, 2 * n), dtype=np.uint64)
        both_n = np.zeros((W, 2 * n), dtype=np.uint64)
        any_n = False
        for L in np.unique(cut):
            L = int(L)
            if L == 0:
                continue
            rows = np.nonzero(cut == L)[0]
            codes = np.empty((rows.size, L), dtype=np.uint8)
            for w in range((L + 31) // 32):
                nb = min(32, L - 32 * w)
                sh = (2 * np.arange(nb)).astype(np.uint64)
                part = ((words[w, rows][:, None] >> sh[None, :]) & np.uint64(3)).astype(np.uint8)
                if nmask is not None:
                    isn = ((np.asarray(nmask, dtype=np.uint64)[w, rows][:, None] >> sh[None, :]) & np.uint64(1)).astype(bool)
                    part[isn] = 4
                codes[:, 32 * w:32 * w + nb] = part
            back = codes[:, ::-1]
            back = np.where(back > 3, 4, 3 - back).astype(np.uint8)
            for grid, at in ((codes, rows), (back, rows + n)):
                w_, _, n_ = pack.pack_codes(grid, W)
                both_w[:, at] = w_
                if n_ is not None:
                    both_n[:, at] = n_
                    any_n = True
        rs = ReadSet(both_w, np.concatenate([cut, cut]).astype(np.uint8), both_n if any_n else None, None,
                     device=self.engine.device)
        for key in self.keys:
            mm, cnt = self.engine.count_best(rs, key, seed_len=28, max_mm_seed=max_mm_seed, max_mm_total=2)
            for half in (slice(0, n), slice(n, 2 * n)):
                m, c = mm[half].astype(np.int32), cnt[half].astype(np.int64)
                undecided |= (m == 255) & (c == 255)
                better = m < best_mm
                same = (m == best_mm) & (m < 255)
                count = np.where(better, c, np.where(same, count + c, count))
                best_mm = np.where(better, m, best_mm)
        return best_mm, count, undecided

    def unique_best_mask(self, words, lens, nmask=None):
        """unique_best over the packed reads words [W, n] / lens / nmask: a boolean per read."""
        mm, cnt, und = self._best_packed(words, lens, nmask, 1)
        return (mm < 255) & (cnt == 1) & ~und

    def exact_hit_mask(self, words, lens, nmask=None):
        """exact_hit over the packed reads: a boolean per read."""
        mm, _, und = self._best_packed(words, lens, nmask, 0)
        return (mm < 255) | und
