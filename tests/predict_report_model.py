"""The rule of predict mode's report in plain Python: what the reference's utils/write_novel_report.py computes up to its
drawing, from the texts of its three input files.

run(novel, table, cluster) walks the reference's own steps over strings, lists and dicts -- the pair correction in file order,
the arm re-type, the per-line facts and groups, the cluster file's blocks, the `while` over the novel list -- and returns the
two files the reference writes (`corrected`, `report`), the arguments it hands to creatPDF per entry (`calls`), the extension
file (`profiles`) and, for the tests of the device calls, the same results as arrays in the layout of include/mirge_amd.h.
Where the reference raises (an IndexError, a KeyError, int('None'), .index() of an absent string) run raises ValueError.
arrays(novel, table, cluster) is what the native reader hands out.  standin(...) is the same route over files, the Python
side of scripts/predict_report_timing.py.
"""
import os
import re

import numpy as np

NONE, BAD = -2 ** 63, -2 ** 63 + 1
NO_GROUP = 0xffffffff
REPORT_HEADER = ("Novel miRNA name,Probability,Chr,Start Pos,End Pos,Strand,Mature miRNA sequence,Arm type,Passenger miRNA sequence,"
                 "Mature miRNA read Count,Passenger miRNA read Count,Precursor miRNA sequence,Precursor miRNA structure\n")
COLUMNS = ("clusterName", "clusterSeq", "stableClusterSeq", "alignedClusterSeq", "seqCount", "readCountSum", "headUnstableLength",
           "tailUnstableLength", "upstreamDistance", "downstreamDistance", "pruned_precusor_seq", "pruned_precusor_str", "armType",
           "pair_state")
ARM_CODE = {"arm5": 0, "arm3": 1, "loop": 2}
MAX_PREC, MAX_SEQ, MAX_PAD = 256, 255, 65535
NAME = re.compile(r"[^:]*:[^:]*:([^:]*):([^_:]+)_([^_:]+)([+-])\Z")


def lines_of(text):
    """readlines(): the '\\n' stays."""
    return re.findall(r"[^\n]*\n|[^\n]+", text)


def whole(cell):
    t = cell.strip()
    return int(t) if re.fullmatch(r"[+-]?[0-9]{1,18}", t) else None


def head_dashes(s):
    return len(s) - len(s.lstrip("-"))


def tail_dashes(s):
    return len(s) - len(s.rstrip("-"))


def output_paths(novel_path, table_path, cluster_path):
    """The reference's names: the table's `_corrected.tsv`; the report next to the cluster file under the novel list's stem."""
    stem = os.path.join(os.path.split(os.path.abspath(cluster_path))[0], "_".join(novel_path.split("_")[:-3]))
    return dict(corrected=table_path[:-4] + "_corrected.tsv", report=stem + "_novel_miRNAs_report.csv",
                profiles=stem + "_novel_miRNAs_report_profiles.tsv")


def parse_novel(text):
    ls = lines_of(text)
    if not ls:
        raise ValueError("the novel list has no header line")
    head = ls[0].strip().split(",")
    ip, ic = head.index("probability"), head.index("clusterName")
    names, prob = [], {}
    for ln in ls[1:]:
        c = ln.strip().split(",")
        if len(c) <= max(ip, ic):
            raise ValueError("the novel list: a line with fewer cells than the header names")
        if c[ic] not in prob:
            names.append(c[ic])
            prob[c[ic]] = c[ip]
    return names, prob


class Table:
    """The screened table's lines, cells and validated facts."""

    def __init__(self, text, listed):
        raw = lines_of(text)
        if not raw:
            raise ValueError("the table has no header line")
        self.header_raw, self.raw = raw[0], raw[1:]
        self.header = raw[0].strip().split("\t")
        self.ix = {k: self.header.index(k) for k in COLUMNS}
        need = max(self.ix.values()) + 1
        self.cells = [ln.strip().split("\t") for ln in self.raw]
        self.n = len(self.cells)
        self.chr, self.strand, self.start, self.end, self.hul, self.tul, self.reads, self.up, self.down = ([] for _ in range(9))
        seen = set()
        for j, c in enumerate(self.cells):
            if len(c) < need:
                raise ValueError("line %d of the table: fewer cells than the header names" % (j + 2))
            m = NAME.match(c[self.ix["clusterName"]])
            s, e = (whole(m.group(2)), whole(m.group(3))) if m else (None, None)
            if s is None or e is None:
                raise ValueError("line %d of the table: clusterName is not <sample>:<cluster>:<chr>:<start>_<end><+|->" % (j + 2))
            if c[self.ix["clusterName"]] in seen:
                raise ValueError("line %d of the table: clusterName is repeated" % (j + 2))
            seen.add(c[self.ix["clusterName"]])
            nums = [whole(c[self.ix[k]]) for k in ("headUnstableLength", "tailUnstableLength", "readCountSum")]
            if None in nums:
                raise ValueError("line %d of the table: headUnstableLength, tailUnstableLength or readCountSum is no whole number" % (j + 2))
            self.chr.append(m.group(1))
            self.strand.append(m.group(4))
            self.start.append(s)
            self.end.append(e)
            self.hul.append(nums[0])
            self.tul.append(nums[1])
            self.reads.append(nums[2])
            for key, dst in (("upstreamDistance", self.up), ("downstreamDistance", self.down)):
                cell = c[self.ix[key]]
                v = NONE if cell == "None" else whole(cell)
                dst.append(BAD if v is None else v)
        for nm in listed:
            if nm not in seen:
                raise ValueError("the novel list names %s, which the table does not hold" % nm)

    def col(self, j, key):
        return self.cells[j][self.ix[key]]


def parse_blocks(text, table, line_of):
    """line -> (state, rows): state 1 read / 2 malformed; rows = (RNA, start, end, count).  A name's last block counts."""
    ls = lines_of(text)
    labels = [i for i, ln in enumerate(ls) if "Cluster Name:" in ln]
    out = {}
    for k, lo in enumerate(labels):
        sub = ls[lo:labels[k + 1]] if k + 1 < len(labels) else ls[lo:]
        words = sub[0].strip().split(" ")
        if len(words) < 3 or words[2] not in line_of:
            continue
        j = line_of[words[2]]
        out[j] = (2, [])
        if len(sub) < 5:
            continue
        dashed, minus = sub[4].strip(), table.strand[j] == "-"
        d_start = table.start[j] - (tail_dashes(dashed) if minus else head_dashes(dashed))
        d_end = table.end[j] + (head_dashes(dashed) if minus else tail_dashes(dashed))
        rows = []
        for item in sub[5:]:
            member = item.split("\t")[0]
            c = item.strip().split("\t")
            count = whole(c[1]) if len(c) >= 2 else None
            if count is None or count < 0:
                rows = None
                break
            start = d_start + (tail_dashes(member) if minus else head_dashes(member))
            end = d_end - (head_dashes(member) if minus else tail_dashes(member))
            rows.append((member.replace("-", "").replace("T", "U"), start, end, count))
        if rows is not None:
            out[j] = (1, rows)
    return out


def retype(seq, structure, cluster_seq):
    """True when the stretch of the structure under clusterSeq (T as U) holds a `(` somewhere before a `)`."""
    rna = cluster_seq.replace("T", "U")
    start = seq.find(rna)
    return re.search(r"\(.*\)", structure[start:start + len(rna)]) is not None


def padded_rows(rows, stable, precursor, start, end, strand):
    """padClusteredList: (padded row, count) and the dashes in front and behind."""
    at = precursor.find(stable)
    if at < 0:
        raise ValueError("the stable sequence %s is not in the precursor" % stable)
    head, tail = at, len(precursor) - at - len(stable)
    p_head, p_tail = (start - head, end + tail) if strand == "+" else (start - tail, end + head)
    out = []
    for seq, r_start, r_end, count in rows:
        before, behind = max(0, r_start - p_head), max(0, p_tail - r_end)
        lead, trail = (before, behind) if strand == "+" else (behind, before)
        out.append(("-" * lead + seq + "-" * trail, count, lead, trail))
    return out


def profile_of(precursor, rows):
    """(per position the summed count of the rows whose character there is the precursor's, total, ragged)."""
    sums = [0] * len(precursor)
    for text, count in rows:
        for p in range(min(len(text), len(precursor))):
            if text[p] == precursor[p]:
                sums[p] += count
    return sums, sum(c for _, c in rows), int(any(len(t) != len(precursor) for t, _ in rows))


def run(novel_text, table_text, cluster_text):
    names, prob = parse_novel(novel_text)
    t = Table(table_text, names)
    n, ix = t.n, t.ix
    line_of = {t.col(j, "clusterName"): j for j in range(n)}
    listed = [t.col(j, "clusterName") in prob for j in range(n)]
    # 1. the pair correction, in file order
    src, touched, head_touched = list(range(n)), [False] * n, False

    def takes(j, i):
        arm = t.col(j, "armType")
        return t.col(j, "pair_state") == "Yes" and arm in ("arm5", "arm3") and arm != t.col(i, "armType")
    for i in range(n):
        if not (listed[i] and t.col(i, "pair_state") == "Yes" and t.up[i] != NONE):
            continue
        if t.up[i] == BAD:
            raise ValueError("line %d of the table: upstreamDistance is no whole number" % (i + 2))
        if t.up[i] <= 44:
            if i == 0:
                head_touched = True
            else:
                touched[i - 1] = True
                if takes(i - 1, i):
                    src[i - 1] = i
        else:
            if t.down[i] in (NONE, BAD):
                raise ValueError("line %d of the table: upstreamDistance exceeds 44 and downstreamDistance is None or no whole number" % (i + 2))
            if t.down[i] <= 44:
                if i + 1 >= n:
                    raise ValueError("line %d of the table: the last line offers its precursor to a line that does not exist" % (i + 2))
                touched[i + 1] = True
                if takes(i + 1, i):
                    src[i + 1] = i
    seq = [t.col(src[j], "pruned_precusor_seq") for j in range(n)]
    structure = [t.col(src[j], "pruned_precusor_str") for j in range(n)]
    # 2. the arm re-type
    retyped = [retype(seq[j], structure[j], t.col(j, "clusterSeq")) and t.col(j, "armType") != "loop" for j in range(n)]
    arm = ["loop" if retyped[j] else t.col(j, "armType") for j in range(n)]
    out = [("\t".join(t.header) + "\n") if head_touched else t.header_raw]
    for j in range(n):
        if not (touched[j] or retyped[j]):
            out.append(t.raw[j])
            continue
        c = list(t.cells[j])
        c[ix["pruned_precusor_seq"]], c[ix["pruned_precusor_str"]], c[ix["armType"]] = seq[j], structure[j], arm[j]
        out.append("\t".join(c) + "\n")
    corrected = "".join(out)
    # 3. the per-line facts and the groups
    pos, stable, groups = [], [], {}
    for j in range(n):
        hd, td = head_dashes(t.col(j, "alignedClusterSeq")), tail_dashes(t.col(j, "alignedClusterSeq"))
        if t.strand[j] == "+":
            pos.append((t.start[j] - hd + t.hul[j], t.end[j] + td - t.tul[j]))
        else:
            pos.append((t.start[j] - td + t.tul[j], t.end[j] + hd - t.hul[j]))
        stable.append(t.col(j, "stableClusterSeq").replace("T", "U"))
        if seq[j] != "None":
            groups.setdefault((seq[j], t.chr[j], t.strand[j]), []).append(j)
    # 5. the blocks
    blocks = parse_blocks(cluster_text, t, line_of)
    # 4. the entries
    remaining, entries, calls, chunks = list(names), [], [], []
    while remaining:
        first = line_of[remaining[0]]
        if seq[first] == "None":
            raise ValueError("line %d of the table: %s is in the novel list and its precursor is None" % (first + 2, remaining[0]))
        members = groups[(seq[first], t.chr[first], t.strand[first])]
        for k in range(0, len(members), 2):
            pair = members[k:k + 2]
            if len(pair) == 1:
                m, p = pair[0], None
            else:
                a, b = pair
                if listed[a] and listed[b]:
                    m, p = (a, b) if t.reads[a] >= t.reads[b] else (b, a)
                elif listed[a] and not listed[b]:
                    m, p = a, b
                else:
                    m, p = b, a
                if arm[p] == "loop":
                    p = None
            for x in (m, p):
                if x is not None and blocks.get(x, (0, None))[0] != 1:
                    raise ValueError("line %d of the table: the cluster file holds no (or a malformed) block of %s" % (x + 2, t.col(x, "clusterName")))
            rows_m = padded_rows(blocks[m][1], stable[m], seq[m], pos[m][0], pos[m][1], t.strand[m])
            rows_p = None if p is None else padded_rows(blocks[p][1], stable[p], seq[m], pos[p][0], pos[p][1], t.strand[p])
            chunks.append((m, p))
            if arm[m] != "loop":
                if not listed[m]:
                    raise ValueError("line %d of the table: %s is the mature one of its pair and is not in the novel list" % (m + 2, t.col(m, "clusterName")))
                entries.append((m, p, rows_m, rows_p))
                total = t.reads[m] + (0 if p is None else t.reads[p])
                calls.append(dict(name="novel_miRNA_%d" % len(entries), probability=prob[t.col(m, "clusterName")], chr=t.chr[m], start=pos[m][0],
                                  end=pos[m][1], strand=t.strand[m], arm=arm[m], mature_reads=t.col(m, "readCountSum"), total_reads=total,
                                  precursor=seq[m], structure=structure[m], mature=stable[m], passenger="None" if p is None else stable[p],
                                  mature_rows=[[r[0], r[1]] for r in rows_m],
                                  passenger_rows="None" if rows_p is None else [[r[0], r[1]] for r in rows_p]))
            for x in pair:
                nm = t.col(x, "clusterName")
                if nm in remaining:
                    remaining.remove(nm)
    # the files
    report, profiles = [REPORT_HEADER], []
    lead, trail, prof, totals, flags, row_off, prof_off = [], [], [], [], [], [0], [0]
    for e, (m, p, rows_m, rows_p) in enumerate(entries):
        c = calls[e]
        report.append(",".join([c["name"], c["probability"], c["chr"], str(c["start"]), str(c["end"]), c["strand"], c["mature"], c["arm"],
                                c["passenger"], c["mature_reads"], "None" if p is None else t.col(p, "readCountSum"), c["precursor"],
                                c["structure"]]) + "\n")
        rows = rows_m + (rows_p or [])
        sums, total, ragged = profile_of(seq[m], [(r[0], r[1]) for r in rows])
        profiles.append(">%s\t%d\t%d\t%d\t%d\n%s\n%s\n%s\n" % (c["name"], len(seq[m]), total, len(rows), ragged, seq[m], structure[m],
                                                                "\t".join(str(s) for s in sums)))
        profiles.extend("%s\t%d\n" % (r[0], r[1]) for r in rows)
        lead.extend(r[2] for r in rows)
        trail.extend(r[3] for r in rows)
        prof.extend(sums)
        totals.append(total)
        host = len(seq[m]) > MAX_PREC or any(len(r[0]) - r[2] - r[3] > MAX_SEQ or max(r[2], r[3]) > MAX_PAD for r in rows)
        flags.append(ragged | (2 if host else 0))
        row_off.append(len(lead))
        prof_off.append(len(prof))
    host_line = [len(seq[j]) > MAX_PREC or len(structure[j]) > MAX_PREC or len(t.col(j, "clusterSeq")) > MAX_SEQ or len(stable[j]) > MAX_SEQ
                 for j in range(n)]
    state = [(1 if touched[j] else 0) | (2 if retyped[j] else 0) | (4 if host_line[j] else 0) | (8 if seq[j] == "None" else 0) |
             (ARM_CODE.get(arm[j], 3) << 4) for j in range(n)]
    return dict(corrected=corrected, report="".join(report), profiles="".join(profiles), calls=calls, n_entries=len(entries), chunks=chunks,
                src=np.array(src, np.uint32), state=np.array(state, np.uint8), pos_adj=np.array(pos, np.int64).reshape(n, 2),
                stable_idx=np.array([seq[j].find(stable[j]) for j in range(n)], np.int32),
                ent_m=np.array([e[0] for e in entries], np.uint32), ent_p=np.array([-1 if e[1] is None else e[1] for e in entries], np.int32),
                row_off=np.array(row_off, np.uint64), prof_off=np.array(prof_off, np.uint64), lead=np.array(lead, np.int32),
                trail=np.array(trail, np.int32), prof=np.array(prof, np.uint64), total=np.array(totals, np.uint64),
                flag=np.array(flags, np.uint8), host_lines=int(sum(host_line)))


def arrays(novel_text, table_text, cluster_text):
    """What the native reader hands out (include/mirge_amd.h, mrg_predict_report_array), as numpy arrays."""
    names, prob = parse_novel(novel_text)
    t = Table(table_text, names)
    n = t.n
    rank_of = {nm: k for k, nm in enumerate(names)}
    flags, rank, text, t_off = [], [], [], [0]
    for j in range(n):
        nm = t.col(j, "clusterName")
        f = (1 if nm in rank_of else 0) | (2 if t.col(j, "pair_state") == "Yes" else 0) | (4 if t.col(j, "pruned_precusor_seq") == "None" else 0)
        f |= ARM_CODE.get(t.col(j, "armType"), 3) << 3
        f |= 32 if t.strand[j] == "-" else 0
        flags.append(f)
        rank.append(rank_of.get(nm, 0xffffffff))
        for key in ("pruned_precusor_seq", "pruned_precusor_str", "clusterSeq", "stableClusterSeq"):
            text.append(t.col(j, key))
            t_off.append(t_off[-1] + len(text[-1]))
    ids, gid3 = {}, np.full((n, 3), NO_GROUP, np.uint32)
    for j in range(n):
        for d in (-1, 0, 1):
            if 0 <= j + d < n:
                gid3[j, d + 1] = ids.setdefault((t.col(j + d, "pruned_precusor_seq"), t.chr[j], t.strand[j]), len(ids))
    blocks = parse_blocks(cluster_text, t, {t.col(j, "clusterName"): j for j in range(n)})
    blk, r_off, rows = [], [0], []
    for j in range(n):
        state, rs = blocks.get(j, (0, []))
        blk.append(state)
        rows.extend(rs)
        r_off.append(len(rows))
    s_off = np.zeros(len(rows) + 1, np.uint64)
    s_off[1:] = np.cumsum([len(r[0]) for r in rows], dtype=np.uint64)
    adj = [[head_dashes(t.col(j, "alignedClusterSeq")), tail_dashes(t.col(j, "alignedClusterSeq")), t.hul[j], t.tul[j]] for j in range(n)]
    return dict(n=n, n_listed=len(names), prob=[prob[nm] for nm in names], flags=np.array(flags, np.uint8), rank=np.array(rank, np.uint32),
                up=np.array(t.up, np.int64), down=np.array(t.down, np.int64), pos=np.array(list(zip(t.start, t.end)), np.int64).reshape(n, 2),
                adj=np.array(adj, np.int32).reshape(n, 4), reads=np.array(t.reads, np.int64), gid3=gid3, t_off=np.array(t_off, np.uint64),
                text="".join(text).encode("ascii"), blk=np.array(blk, np.uint8), r_off=np.array(r_off, np.uint64),
                row_start=np.array([r[1] for r in rows], np.int64), row_end=np.array([r[2] for r in rows], np.int64),
                row_count=np.array([r[3] for r in rows], np.int64), row_soff=s_off, row_text="".join(r[0] for r in rows).encode("ascii"))


def standin(novel_path, table_path, cluster_path):
    """The same route in Python over the same three files: reads them, runs the rule, writes the three output files."""
    texts = []
    for p in (novel_path, table_path, cluster_path):
        with open(p) as fh:
            texts.append(fh.read())
    res = run(*texts)
    paths = output_paths(novel_path, table_path, cluster_path)
    for key, p in paths.items():
        with open(p, "w") as fh:
            fh.write(res[key])
    return res["n_entries"]
