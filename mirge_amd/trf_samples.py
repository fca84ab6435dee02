"""Per-sample tRF reports and their density-peak clustering for `-trf` (W2C = writeDataToCSV.py :802-1088):
`<outdir>/tRFs.samples.tmp/<sample>.{potential_tRFs.report, potential_tRFs.summary.report,
potential_tRFs.clusters.detail, tRFs.report.tsv}` from the trfContentDic that `trf.write_trf_tables` leaves.

Every (sample, tRNA) block of the report is clustered with Rodriguez-Laio density peaks (W2C:417-533, :877-961:
gaussian, dc = 3, centers at rho >= 5 and delta >= 8).  The O(n^2) parts run for all blocks of a run at once
through an injectable `peaks(off, codes, nmask, span, rpm, max_len, ktab)` backend -- Engine.trf_peaks on the GPU,
a numpy model in the CPU tests -- whose result has .rho, .max_dis, .min_distance(rank) and .border(labels,
bord_off); this module does the O(n) rest.

Restated quirks: rows longer than their template (overhanging poly-T trailers) count in the block sums but are
left out of the rows and the clustering; load_data_new skips an empty block, which shifts the pairing of blocks
and names; abundantSeq is always the center's; a top row that is not a center keeps label -1.  Pinned: the rank
order is a stable sort of -rho (the reference's np.argsort is not stable for large float32 arrays in NumPy 2);
`round` is Python 3's, as in trf.py (Python 2 rounds exact decimal halves away from zero).
"""
import math
import os

import numpy as np

DC, RHOMIN, DELTAMIN, RP100K_CUTOFF = 3.0, 5.0, 8.0, 10.0  # W2C:877
MAX_TEMPLATE = 255


def gaussian_table(dc=DC):
    """K[d] = math.exp(-(d / dc) ** 2) (W2C:486) for every integer distance until it underflows to 0.0."""
    k = []
    for d in range(4096):
        v = math.exp(-(float(d) / dc) ** 2)
        if v == 0.0:
            break
        k.append(v)
    return np.array(k, dtype=np.float64)


# ---------------------------------------------------------------- helpers (W2C:20-33, :71-73, :233-246, :535-544)
def dash_count(seq):
    return len(seq) - len(seq.lstrip("-")), len(seq) - len(seq.rstrip("-"))


def remove_dash(seq):
    h, t = dash_count(seq)
    return seq[h:len(seq) - t]


def detect_mismatch(target_seq, template_seq, position_tmp):
    state, pos = "N", []
    start, end = int(position_tmp.split(":")[0]) - 1, int(position_tmp.split(":")[1]) - 1
    tmp = template_seq[start:end + 1]
    for i in range(len(target_seq)):
        if target_seq[i] != tmp[i]:
            state = "Y"
            pos.append(str(start + 1 + i))
    return state, ",".join(pos)


def load_data_new(content):
    """W2C:394-415 over the report's lines: one list of rows (aligned seq, type, count, RP100K) per non-empty
    block."""
    label = [-1] + [k for k, item in enumerate(content) if "mature tRNA" in item or "primary tRNA trailer" in item]
    out = []
    for i in range(len(label) - 1):
        rows = []
        for line in content[label[i] + 2:label[i + 1]]:
            d = line.strip().split("\t")
            rows.append((d[0], d[1], int(d[2]), float(d[3])))
        if rows:
            out.append(rows)
    return out


# ---------------------------------------------------------------- reports (W2C:802-874)
def sample_trf_dic(trfContentDic, sampleList, trnaStruDic, pretrnaNameSeqDic):
    """W2C:805-822: sample -> tRNA -> [(count, start, read, dashed read, tRF type, RP100K)]."""
    out = {s: {} for s in sampleList}
    for read, rec in trfContentDic.items():
        for i, s in enumerate(sampleList):
            if rec["count"][i] > 0:
                for name, e in rec.items():
                    if name in ("uid", "RPM", "count"):
                        continue
                    template = trnaStruDic[name]["seq"] if "pre" not in name else pretrnaNameSeqDic[name]
                    filled = e["start"] * "-" + read + (len(template) - e["start"] - len(read)) * "-"
                    out[s].setdefault(name, []).append((rec["count"][i], e["start"], read, filled, e["tRFType"],
                                                        rec["RPM"][i]))
    return out


def sample_reports(tdic, trnaStruDic, trnaAAanticodonDic, pretrnaNameSeqDic):
    """W2C:823-874 for one sample: (lines of .potential_tRFs.report, text of .potential_tRFs.summary.report)."""
    summary = ["amino acid\tCounts\tRP100K\tUnique reads\n"]
    aa_list, aa_dic = [], {}
    lines = []
    sums = []
    for name, rows in tdic.items():
        sums.append((sum([r[0] for r in rows]), name, sum([r[5] for r in rows])))
    sums.sort(reverse=True)

    def add(key, r):
        aa_dic[key][0] += r[0]
        aa_dic[key][1] += r[5]
        aa_dic[key][2] += 1
    for read_sum, name, rpm_sum in sums:
        aa = trnaAAanticodonDic[name]["aaType"]
        if "pre_" in name:
            aa = "pre:" + aa
        keys = [aa + " tRF-1"] if "pre:" in aa else [aa + " 5'", aa + " 3'", aa + " other"]
        for k in keys:
            if k not in aa_list:
                aa_list.append(k)
                aa_dic[k] = [0, 0, 0]
        rows = sorted(tdic[name], reverse=True)
        lines.append(name + "\tread count sum:" + str(read_sum) + "\tRP100K sum:" + "%.3f" % round(rpm_sum, 3) + "\n")
        if "pre" not in name:
            template, ttype = trnaStruDic[name]["seq"], "mature tRNA"
        else:
            template, ttype = pretrnaNameSeqDic[name], "primary tRNA trailer"
        for r in rows:
            if len(r[3]) != len(template):
                continue
            lines.append(r[3] + "\t" + r[4] + "\t" + str(r[0]) + "\t" + "%.3f" % round(r[5], 3) + "\n")
            if "pre:" in aa:
                add(aa + " tRF-1", r)
            else:
                left, right = dash_count(r[3])
                add(aa + (" 5'" if left <= 2 else " 3'" if right <= 2 else " other"), r)
        lines.append(template + "\t" + ttype + "\t" + str(read_sum) + "\t" + "%.3f" % round(rpm_sum, 3) + "\n")
    for k in aa_list:
        summary.append("\t".join([k, str(aa_dic[k][0]), "%.3f" % round(aa_dic[k][1], 3), str(aa_dic[k][2])]) + "\n")
    return lines, "".join(summary)


# ---------------------------------------------------------------- rows -> device layout
_CODE = np.zeros(256, dtype=np.uint64)
for _c, _v in zip(b"ACGT", range(4)):
    _CODE[_c] = _v
_VALID = np.zeros(256, dtype=bool)
_VALID[list(b"ACGTN-")] = True


class Group:
    """One (sample, tRNA) block: its rows as the reference's readInforDic, and as a character matrix."""

    def __init__(self, rows):
        self.seqs = [r[0] for r in rows]
        self.types = [r[1] for r in rows]
        self.counts = [r[2] for r in rows]
        self.rpm = np.array([r[3] for r in rows], dtype=np.float64)
        self.n = len(rows)
        self.L = len(self.seqs[0])
        if any(len(s) != self.L for s in self.seqs):
            raise ValueError("trf_samples: rows of one block differ in length")
        self.chars = np.frombuffer("".join(self.seqs).encode("ascii"), dtype=np.uint8).reshape(self.n, self.L)
        if not _VALID[self.chars].all():
            raise ValueError("trf_samples: a row holds a character other than A, C, G, T, N or '-'")
        present = self.chars != ord("-")
        self.first = present.argmax(axis=1).astype(np.int64) + 1
        self.last = self.L - present[:, ::-1].argmax(axis=1).astype(np.int64)

    def pack(self, W):
        """2-bit codes and N mask, [W][n] words each, of the template frame (see include/mirge_amd.h)."""
        wide = np.zeros((self.n, W * 32), dtype=np.uint8)
        wide[:, :self.L] = self.chars
        shifts = (2 * np.arange(32, dtype=np.uint64))[None, None, :]
        code = (_CODE[wide].reshape(self.n, W, 32) << shifts).sum(axis=2, dtype=np.uint64)
        nbit = ((wide == ord("N")).astype(np.uint64).reshape(self.n, W, 32) << shifts).sum(axis=2, dtype=np.uint64)
        return code.T, nbit.T

    def distance_to(self, c, rows):
        """getDistance (W2C:434-440) of the given rows (0-based) to row c."""
        ch = self.chars[rows]
        sub = ((ch != self.chars[c]) & (ch != ord("-")) & (self.chars[c] != ord("-"))[None, :]).sum(axis=1)
        return np.abs(self.first[rows] - self.first[c]) + np.abs(self.last[rows] - self.last[c]) + sub


def layout(groups):
    """The groups as the device arrays of include/mirge_amd.h: (off, codes, nmask or None, span, rpm, max_len)."""
    off = np.zeros(len(groups) + 1, dtype=np.uint32)
    off[1:] = np.cumsum([g.n for g in groups])
    n_all = int(off[-1])
    max_len = max([g.L for g in groups] + [1])
    if max_len > MAX_TEMPLATE:   # (the device entry points refuse it too: MRG_ERR_ARG)
        raise ValueError("trf_samples: a template of %d nt: density peaks take templates of at most %d nt"
                         % (max_len, MAX_TEMPLATE))
    W = (max_len + 31) // 32
    codes, nmask = np.zeros((W, n_all), dtype=np.uint64), np.zeros((W, n_all), dtype=np.uint64)
    span, rpm = np.zeros(n_all, dtype=np.uint16), np.zeros(n_all, dtype=np.float64)
    for k, g in enumerate(groups):
        a, b = int(off[k]), int(off[k + 1])
        codes[:, a:b], nmask[:, a:b] = g.pack(W)
        span[a:b] = (g.first | (g.last << 8)).astype(np.uint16)
        rpm[a:b] = g.rpm
    return off, codes, nmask if nmask.any() else None, span, rpm, max_len


def run_peaks(groups, peaks):
    """All groups through the backend: rank, centers, labels, border densities.  Returns one dict per group
    with rho, delta, nneigh, sort_rho_idx (the reference's arrays, index 0 = the dummy), cl, NCLUST, ccenter
    and bord_rho."""
    args = layout(groups)
    return peaks_results(args[0], peaks(*args, gaussian_table()))


def peaks_results(off, state, device_rank=False):
    """run_peaks after the rho pass, for groups given by their row offsets alone.  The rank order is a stable argsort
    of -rho per group here, as run_peaks has always done; with device_rank it is the backend's (state.rank():
    mrg_trf_rank on the GPU, where the rank then stays for min_distance(None); only the array route asks for it).
    rho is downloaded either way: the label pass below reads it."""
    n_groups, n_all = len(off) - 1, int(off[-1])
    sizes = np.diff(np.asarray(off).astype(np.int64))
    rho_all = np.asarray(state.rho, dtype=np.float32)
    max_dis = np.asarray(state.max_dis)
    # min_distance's rank order (W2C:521): stable sort of -rho, the dummy index 0 (rho = -1) last
    from_backend = bool(device_rank)
    res, rank = [], (np.asarray(state.rank()) if from_backend else np.zeros(n_all, dtype=np.uint32))
    for k in range(n_groups):
        a, b = int(off[k]), int(off[k + 1])
        rho = np.empty(int(sizes[k]) + 1, dtype=np.float32)
        rho[0] = -1.0
        rho[1:] = rho_all[a:b]
        if from_backend:
            order = np.zeros(int(sizes[k]) + 1, dtype=np.int64)
            order[:-1] = rank[a:b].astype(np.int64) + 1
        else:
            order = np.argsort(-rho, kind="stable")
            assert order[-1] == 0
            rank[a:b] = order[:-1] - 1
        res.append({"rho": rho, "sort_rho_idx": order, "max_dis": int(max_dis[k])})
    delta_all, nneigh_all = state.min_distance(None if from_backend else rank)
    bord_off = np.zeros(n_groups + 1, dtype=np.uint32)
    labels = np.zeros(n_all, dtype=np.int32)
    for k in range(n_groups):
        gn = int(sizes[k])
        a, b = int(off[k]), int(off[k + 1])
        r = res[k]
        top = int(r["sort_rho_idx"][0])
        dl = np.empty(gn + 1, dtype=np.float64)
        dl[0] = 0.0
        dl[1:] = delta_all[a:b]
        dl[top] = -1.0
        dl[top] = dl.max()                                           # W2C:532
        nn = np.zeros(gn + 1, dtype=np.int32)
        nn[1:] = nneigh_all[a:b] + 1
        nn[top] = 0
        rho = r["rho"]
        delta = dl.astype(np.float32)
        # cluster centers (W2C:883-893)
        centers = (np.nonzero((rho[1:] >= RHOMIN) & (delta[1:] >= DELTAMIN))[0] + 1).tolist()
        cl = np.zeros(gn + 1) - 1
        ccenter = {}
        for c, idx in enumerate(centers, 1):
            cl[idx] = c
            ccenter[c] = idx
        nclust = len(centers)
        if nclust == 0 and float(delta[1:].max()) <= DELTAMIN and float(rho[1:].max()) >= RHOMIN:  # W2C:895-908
            nclust = 1
            idx = int(np.argmax(rho[1:])) + 1
            cl[idx] = 1
            ccenter[1] = idx
        # assignation (W2C:910-912): in rank order, a row takes its nearest denser neighbour's label
        cl_l, order, nn_l = cl.tolist(), r["sort_rho_idx"].tolist(), nn.tolist()
        for i in range(gn):
            s = order[i]
            if cl_l[s] == -1:
                cl_l[s] = cl_l[nn_l[s]]
        cl = np.array(cl_l).astype(np.int32)
        labels[a:b] = cl[1:]
        if nclust > 1:
            bord_off[k + 1] = nclust + 1
        r.update(delta=delta, nneigh=nn, cl=cl, NCLUST=nclust, ccenter=ccenter)
    bord_off = np.cumsum(bord_off, dtype=np.uint64).astype(np.uint32)
    bord_all = state.border(labels, bord_off) if int(bord_off[-1]) else np.zeros(0, dtype=np.float32)
    for k, r in enumerate(res):
        r["bord_rho"] = np.asarray(bord_all[int(bord_off[k]):int(bord_off[k + 1])], dtype=np.float32)
    return res


def cluster_text(name, g, r):
    """W2C:914-1056 for one group after the peaks: (.clusters.detail text, clusterContentList, sumRP100K)."""
    n, cl, nclust, ccenter = g.n, r["cl"], r["NCLUST"], r["ccenter"]
    rho = r["rho"]
    halo = np.zeros(n + 1)
    halo[:] = cl
    if nclust >= 1:
        # distance of each row to the center of its cluster (label -1: none, the reference's KeyError)
        dcen = np.zeros(n + 1, dtype=np.int64)
        for c, idx in ccenter.items():
            sel = np.nonzero(cl[1:] == c)[0]
            dcen[sel + 1] = g.distance_to(idx - 1, sel)
        has = cl >= 1
        has[0] = False
        if nclust > 1:
            bord = r["bord_rho"]
            slot = np.where(cl < 0, cl + nclust + 1, cl)
            below = rho < bord[slot]
            below[0] = False
            halo[below] = 0
        halo[has & (dcen > DELTAMIN)] = 0
    else:
        halo[:] = 0
    seqs, types, counts, rpm = g.seqs, g.types, g.counts, g.rpm.tolist()
    con = name + ":\n"
    sum_count, sum_rpm = 0, 0.0
    core_c, halo_c, core_r, halo_r = [], [], [], []
    n_out = 1
    content = []
    if nclust >= 1:
        cl_l, halo_l = cl.tolist(), halo.tolist()
        members, cores = {}, {}
        for j in range(1, n + 1):
            members.setdefault(cl_l[j], []).append(j)
            cores.setdefault(halo_l[j], []).append(j)
        for i in range(1, nclust + 1):
            center = ccenter[i]
            sel = cores.get(i, [])
            nc, nh = len(members.get(i, [])), len(sel)
            th_c, th_r = 0, 0.0
            for j in members.get(i, []):
                if halo_l[j] != i:
                    th_c += counts[j - 1]
                    th_r += rpm[j - 1]
            tc_c, tc_r = 0, 0.0
            for j in sel:
                tc_c += counts[j - 1]
                tc_r += rpm[j - 1]
            if tc_c > 0:
                cseq, ctype = seqs[center - 1], types[center - 1]
                head, tail = dash_count(cseq)
                pos = ":".join([str(head + 1), str(len(cseq) - tail)])
                con += ("Cluster: %d Total Read Count in Core: %d Total Read Count in Halo: %d Total RP100K in Core: "
                        "%.2f Total RP100K in Halo: %.2f Center Index: %d Elements: %d Core: %d Halo: %d\n"
                        % (n_out, tc_c, th_c, tc_r, th_r, center, nc, nh, nc - nh))
                con += "Center:\n"
                con += "%s\t%s\t%d\t%.2f\n" % (cseq, ctype, counts[center - 1], rpm[center - 1])
                a_c, a_r = counts[center - 1], 0.0 + rpm[center - 1]
                for j in sel:
                    if j != center:
                        con += "%s\t%s\t%d\t%.2f\n" % (seqs[j - 1], types[j - 1], counts[j - 1], rpm[j - 1])
                        a_c += counts[j - 1]
                        a_r += rpm[j - 1]
                con += "**********************************\n"
                content.append((remove_dash(cseq), ctype, pos, a_c, a_r))
                n_out += 1
            sum_count += th_c
            sum_count += tc_c
            sum_rpm += th_r
            sum_rpm += tc_r
            core_c.append(tc_c)
            halo_c.append(th_c)
            core_r.append(tc_r)
            halo_r.append(th_r)
    else:
        for j in range(n):
            sum_count += counts[j]
            sum_rpm += rpm[j]
    con += "Summary:\nNumber of Clusters: %d\n" % (n_out - 1)
    con += "total Read Count : %d\n" % sum_count
    con += "total RP100K: %.2f\n" % sum_rpm
    con += "total Cluster Core Read Count: %s=%d\n" % ("+".join(str(x) for x in core_c), sum(core_c))
    con += "total Cluster Core RP100K: %s=%.3f\n" % ("+".join(str(x) for x in core_r), sum(core_r))
    con += "total Cluster Halo Read Count: %s=%d\n" % ("+".join(str(x) for x in halo_c), sum(halo_c))
    con += "total Cluster Halo RP100K: %s=%.3f\n" % ("+".join(str(x) for x in halo_r), sum(halo_r))
    con += "##################################\n"
    return con, content, sum_rpm


def write_trf_samples(outputdir, sampleList, trfContentDic, tables, pretrnaNameSeqDic, peaks):
    """W2C:802-1088: the four files of every sample under <outputdir>/tRFs.samples.tmp/.  `tables` is
    trf.load_trf_tables' dict; `peaks` the density-peak backend (engine_peaks(engine) on the GPU)."""
    stru, aa_dic = tables["trnaStruDic"], tables["trnaAAanticodonDic"]
    tdir = os.path.join(outputdir, "tRFs.samples.tmp")
    os.makedirs(tdir, exist_ok=True)
    sdic = sample_trf_dic(trfContentDic, sampleList, stru, pretrnaNameSeqDic)
    per_sample, groups = [], []
    for sample in sampleList:
        lines, summary = sample_reports(sdic[sample], stru, aa_dic, pretrnaNameSeqDic)
        with open(os.path.join(tdir, sample + ".potential_tRFs.summary.report"), "w") as fh:
            fh.write(summary)
        with open(os.path.join(tdir, sample + ".potential_tRFs.report"), "w") as fh:
            fh.write("".join(lines))
        blocks = load_data_new(lines)
        names = [line.split("\t")[0] for line in lines if "RP100K sum:" in line]
        per_sample.append((sample, names, len(groups), len(blocks)))
        groups += [Group(rows) for rows in blocks]
    res = run_peaks(groups, peaks) if groups else []
    for sample, names, g0, nb in per_sample:
        _write_clusters(tdir, sample, ((names[k], groups[g0 + k], res[g0 + k]) for k in range(nb)), stru, pretrnaNameSeqDic)
    return tdir


def _write_clusters(tdir, sample, named_groups, stru, pretrnaNameSeqDic):
    """W2C:914-1088 for one sample: .clusters.detail and .tRFs.report.tsv from (name, group, peaks result) triples."""
    unified_sel, names_sel, name_dic = [], [], {}
    with open(os.path.join(tdir, sample + ".potential_tRFs.clusters.detail"), "w") as out1:
        for name, group, r in named_groups:
            con, content, sum_rpm = cluster_text(name, group, r)
            out1.write(con)
            name_dic[name] = content
            if sum_rpm >= RP100K_CUTOFF:
                names_sel.append(name)
                if "pre" in name:
                    name = "_".join(name.split("_")[1:-1])
                if name not in unified_sel:
                    unified_sel.append(name)
    with open(os.path.join(tdir, sample + ".tRFs.report.tsv"), "w") as out2:
        out2.write("tRNA name\ttRNA sequence\ttRF sequence\ttRF mismatch\ttRF type\ttRF coordinate\tRead count\t"
                   "RP100K\n")
        for t in unified_sel:
            if t in names_sel:
                seq = stru[t]["seq"]
                for c in name_dic[t]:
                    st, pos = detect_mismatch(c[0], seq, c[2])
                    out2.write(t + "\t" + seq + "\t" + c[0] + "\t" + ":".join([st, pos]) + "\t" + c[1] + "\t" + c[2]
                               + "\t" + str(c[3]) + "\t" + "%.2f" % round(c[4], 2) + "\n")
            pre = "pre_" + t + "_trailer"
            if pre in names_sel:
                seq = pretrnaNameSeqDic[pre]
                for c in name_dic[pre]:
                    new_pos = ":".join([c[2].split(":")[0], str(int(c[2].split(":")[1]) - 3)])
                    st, pos = detect_mismatch(c[0][:-3], seq, new_pos)
                    out2.write(t + "\t" + seq + "\t" + c[0] + "\t" + ":".join([st, pos]) + "\t" + c[1] + "\t" + c[2]
                               + "\t" + str(c[3]) + "\t" + "%.2f" % round(c[4], 2) + "\n")


def engine_peaks(engine):
    """The density-peak backend on the GPU."""
    return engine.trf_peaks


# ---------------------------------------------------------------- the array route (mrg_trf_sample_groups)
class _Lazy:
    """A read-only sequence whose items are made when they are asked for."""

    def __init__(self, n, make):
        self.n, self.make = n, make

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        if not -self.n <= i < self.n:
            raise IndexError(i)
        return self.make(i % self.n)


_BASES = np.frombuffer(b"ACGT", dtype=np.uint8)


class ArrayGroup:
    """Group's stand-in on the rows [a, b) of the device layout (host copies): what peaks_results' label pass and
    cluster_text ask of a group.  `chars` is decoded from the packed rows; a row becomes a string only when
    cluster_text prints it."""

    def __init__(self, codes, nmask, span, rpm, rows, a, b, L):
        from .trf import TRF_TYPES
        self.n, self.L = b - a, int(L)
        cols = np.arange(self.L)
        sh = (2 * (cols & 31)).astype(np.uint64)[None, :]
        self.chars = _BASES[((codes[cols >> 5, a:b].T >> sh) & np.uint64(3)).astype(np.intp)]
        if nmask is not None:
            self.chars[((nmask[cols >> 5, a:b].T >> sh) & np.uint64(1)).astype(bool)] = ord("N")
        self.first = (span[a:b] & 0xFF).astype(np.int64)
        self.last = (span[a:b] >> 8).astype(np.int64)
        self.chars[(cols[None, :] + 1 < self.first[:, None]) | (cols[None, :] + 1 > self.last[:, None])] = ord("-")
        self.rpm = np.asarray(rpm[a:b], dtype=np.float64)
        self.counts = rows[a:b, 1].tolist()
        types = rows[a:b, 2]
        self.types = _Lazy(self.n, lambda i: TRF_TYPES[types[i]])
        self.seqs = _Lazy(self.n, lambda i: self.chars[i].tobytes().decode("ascii"))

    distance_to = Group.distance_to


def layout_peaks(fn):
    """A `peaks(off, codes, nmask, span, rpm, max_len, ktab)` backend (Engine.trf_peaks, the tests' model) as the
    `peaks(groups, ktab)` backend of write_trf_samples_arrays."""
    return lambda g, ktab: fn(g.off, g.codes, g.nmask, g.span, g.rpm, g.max_len, ktab)


def engine_groups(engine, device=None):
    """The `groups` backend on the GPU.  device: (words, lens, nmask, quant) tensors that already hold the host arrays
    (a single-process run's ReadSet), used in their place."""
    def groups(st, rec, words, lens, nmask, quant, denom, timings=None):
        if device is not None:
            words, lens, nmask, quant = device
        return engine.trf_sample_groups(st, rec, words, lens, nmask, quant, denom, timings=timings)
    return groups


def engine_peaks_groups(engine):
    """The density-peak backend on the device tensors of engine_groups' result."""
    return engine.trf_peaks_groups


def write_trf_sample_reports(tdir, sampleList, st, et, g, rec, words, lens, nmask, quant, denom):
    """<sample>.potential_tRFs.report and .summary.report of every sample from the arrays and the tables of the
    `groups` backend, by the native writer (mrg_write_trf_sample_reports): the files sample_reports gives."""
    import ctypes as C

    from . import _native
    lib = _native.load()
    words = np.ascontiguousarray(words, dtype=np.uint64)
    W, n = words.shape
    lens = np.ascontiguousarray(lens, dtype=np.uint8)
    nm = None if nmask is None else np.ascontiguousarray(nmask, dtype=np.uint64)
    quant = np.ascontiguousarray(quant, dtype=np.uint32).reshape(n, -1)
    S = len(sampleList)
    rec = np.ascontiguousarray(rec, dtype=np.int32).reshape(-1, 12)
    denom = np.ascontiguousarray(denom, dtype=np.uint64)
    if quant.shape[1] != S or denom.shape[0] != S:
        raise ValueError("write_trf_sample_reports: quant [n, S] and denom [S] must match the samples")
    entries = np.ascontiguousarray(st.entries, dtype=np.int32)
    blocks = np.ascontiguousarray(g.blocks, dtype=np.int32).reshape(-1, 6)
    sums = np.ascontiguousarray(g.block_sums, dtype=np.uint64)
    rows = np.ascontiguousarray(g.rows, dtype=np.uint32).reshape(-1, 3)
    paths = (C.c_char_p * (2 * S))(*[os.fsencode(os.path.join(tdir, s + suffix)) for s in sampleList
                                      for suffix in (".potential_tRFs.report", ".potential_tRFs.summary.report")])

    def strings(items):
        return (C.c_char_p * max(len(items), 1))(*[None if x is None else x.encode() for x in items])
    _native.check(lib.mrg_write_trf_sample_reports(
        paths, S, denom.ctypes.data, words.ctypes.data, W, n, lens.ctypes.data, None if nm is None else nm.ctypes.data, n,
        quant.ctypes.data, rec.ctypes.data, rec.shape[0], entries.ctypes.data, strings(et.names), strings(st.templates),
        strings(st.aa_types), entries.shape[0], int(st.n_names), blocks.ctypes.data, sums.ctypes.data, blocks.shape[0],
        rows.ctypes.data, rows.shape[0]))


def write_trf_cluster_reports(tdir, sampleList, g, names, group_len, group_sample, stru, pretrnaNameSeqDic, labels, core, order,
                              nclust, cen_off, centers, tallies):
    """<sample>.potential_tRFs.clusters.detail and .tRFs.report.tsv of every sample from the downloaded layout of the `groups`
    backend and the arrays of assign() / halo(), by the native writer (mrg_write_trf_cluster_reports): the files
    _write_clusters gives.  names[k] = the name group k is paired with.  Names and templates are resolved per group here;
    a lookup the record route would miss raises its KeyError before a file is written."""
    import ctypes as C

    from . import _native
    lib = _native.load()
    G, n = len(names), int(g.off[-1])
    max_len = max(int(g.max_len), 1)
    W = (max_len + 31) // 32
    if n:
        codes = np.ascontiguousarray(g.codes, dtype=np.uint64).reshape(W, -1)
        nm = None if g.nmask is None else np.ascontiguousarray(g.nmask, dtype=np.uint64).reshape(W, -1)
        span, rpm = np.ascontiguousarray(g.span, dtype=np.uint16), np.ascontiguousarray(g.rpm, dtype=np.float64)
        rows = np.ascontiguousarray(g.rows, dtype=np.uint32).reshape(-1, 3)
    else:
        codes, nm, span, rpm, rows = np.zeros((W, 1), np.uint64), None, np.zeros(1, np.uint16), np.zeros(1), np.zeros((1, 3), np.uint32)
    off = np.ascontiguousarray(g.off, dtype=np.uint32)
    per_name = {}
    for name in set(names):
        per_name[name] = ("_".join(name.split("_")[1:-1]) if "pre" in name else name,
                          stru[name]["seq"] if name in stru else None, pretrnaNameSeqDic.get(name))

    def strings(items):
        return (C.c_char_p * max(len(items), 1))(*[None if x is None else x.encode() for x in items])
    arrays = [np.ascontiguousarray(x, dtype=dt) for x, dt in
              ((group_sample, np.int32), (group_len, np.int32), (labels, np.int32), (core, np.uint8), (order, np.uint32),
               (nclust, np.uint32), (cen_off, np.uint32), (centers, np.uint32), (tallies, np.uint64))]
    gs, gl, lab, co, order, nclust, cen_off, centers, tallies = arrays
    if not (len(gs) == len(gl) == len(nclust) == G == len(off) - 1 == len(cen_off) - 1 and len(lab) == len(co) == len(order) == n
            and len(centers) == int(cen_off[-1]) and tallies.size == 4 * len(centers) and len(span) >= n and len(rpm) >= n
            and rows.shape[0] >= n and codes.shape[1] >= n):
        raise ValueError("write_trf_cluster_reports: the arrays do not match the groups")
    paths = (C.c_char_p * (2 * len(sampleList)))(*[os.fsencode(os.path.join(tdir, s + suffix)) for s in sampleList
                                                    for suffix in (".potential_tRFs.clusters.detail", ".tRFs.report.tsv")])
    status = np.zeros(2, dtype=np.int64)
    _native.check(lib.mrg_write_trf_cluster_reports(
        paths, len(sampleList), codes.ctypes.data, None if nm is None else nm.ctypes.data, max_len, codes.shape[1],
        span.ctypes.data, rpm.ctypes.data, rows.ctypes.data, n, off.ctypes.data, G, gs.ctypes.data, gl.ctypes.data,
        strings(names), strings([per_name[x][0] for x in names]), strings([per_name[x][1] for x in names]),
        strings([per_name[x][2] for x in names]), lab.ctypes.data, co.ctypes.data, order.ctypes.data, nclust.ctypes.data,
        cen_off.ctypes.data, centers.ctypes.data, tallies.ctypes.data, status.ctypes.data))
    if status[0] == 1:
        raise KeyError(names[int(status[1])])
    if status[0] == 2:
        raise IndexError("string index out of range")


def write_trf_samples_arrays(outputdir, sampleList, et, st, rec, words, lens, nmask, quant, denom, tables, pretrnaNameSeqDic,
                             groups, peaks, timings=None, device_rank=False, device_labels=False):
    """write_trf_samples from the arrays: the four files of every sample under <outputdir>/tRFs.samples.tmp/, byte for
    byte, without a Python object per read.  et / st = trf.entry_tables / trf.sample_tables; rec = the rows of
    Engine.trf_classify in the order of the tsv (columnar.write_trf_tables returns them); words / lens / nmask /
    quant = the host arrays of the reads; denom[s] = maturetrnaReads + pretrnaReads.  `groups(st, rec, words, lens,
    nmask, quant, denom, timings=)` is the block backend (engine_groups(engine) on the GPU, tests/trf_groups_model.py
    in the CPU tests), `peaks(groups' result, ktab)` the density-peak backend (engine_peaks_groups(engine), or
    layout_peaks(fn) around a backend of write_trf_samples); device_rank: take the rank order from that backend's
    rank() (mrg_trf_rank) instead of the host argsort.  The two report files are written natively.  device_labels: the
    centres, labels and halos come from that backend too (rank(), min_distance(None), assign(), border(None, bord_off),
    halo(): mrg_trf_assign / mrg_trf_halo on the GPU) and .clusters.detail / .tRFs.report.tsv from the native writer
    (mrg_write_trf_cluster_reports), with no Python per row or cluster; without it the label pass of the peaks and those
    two files walk the groups here, on ArrayGroup."""
    import time
    stru = tables["trnaStruDic"]
    rec = np.asarray(rec).reshape(-1, 12)
    t0 = time.perf_counter()
    g = groups(st, rec, words, lens, nmask, quant, denom, timings=timings)
    if g.no_template_row is not None:      # what sample_trf_dic raises at the first such read, before anything is written
        raise et.errors[(int(rec[g.no_template_row, 1]), "length")]
    if g.max_len > MAX_TEMPLATE:
        raise ValueError("trf_samples: a template of %d nt: density peaks take templates of at most %d nt"
                         % (g.max_len, MAX_TEMPLATE))
    t1 = time.perf_counter()
    tdir = os.path.join(outputdir, "tRFs.samples.tmp")
    os.makedirs(tdir, exist_ok=True)
    write_trf_sample_reports(tdir, sampleList, st, et, g, rec, words, lens, nmask, quant, denom)
    t2 = time.perf_counter()
    off = np.asarray(g.off, dtype=np.uint32)
    n_groups = len(off) - 1
    blocks, pairs = np.asarray(g.blocks).reshape(-1, 6), np.asarray(g.groups).reshape(-1, 2)
    if device_labels:
        entries = np.asarray(st.entries)
        nclust, cen_off, centers = np.zeros(0, dtype=np.uint32), np.zeros(1, dtype=np.uint32), np.zeros(0, dtype=np.uint32)
        labels, core, order, tallies = np.zeros(0, np.int32), np.zeros(0, np.uint8), np.zeros(0, np.uint32), np.zeros((0, 4), np.uint64)
        if n_groups:
            state = peaks(g, gaussian_table())
            state.rank()
            state.min_distance(None)
            nclust, cen_off, centers = state.assign()
            slots = np.where(np.asarray(nclust) > 1, np.asarray(nclust).astype(np.uint64) + 1, 0)
            bord_off = np.zeros(n_groups + 1, dtype=np.uint32)
            bord_off[1:] = np.cumsum(slots, dtype=np.uint64)
            state.border(None, bord_off)
            # (the read counts: the backend's own device copy where it has one)
            core, order, tallies = state.halo(None if getattr(state, "counts_d", None) is not None
                                              else np.asarray(g.rows).reshape(-1, 3)[:, 1])
            labels = state.labels()
        t3 = time.perf_counter()
        if n_groups:
            own, paired = blocks[pairs[:, 0]], blocks[pairs[:, 1]]
            names = [et.names[e] for e in paired[:, 1].tolist()]
            group_len, group_sample = entries[own[:, 1], 1], own[:, 0]
        else:
            names, group_len, group_sample = [], np.zeros(0, np.int32), np.zeros(0, np.int32)
        write_trf_cluster_reports(tdir, sampleList, g, names, group_len, group_sample, stru, pretrnaNameSeqDic, labels, core, order,
                                  nclust, cen_off, centers, tallies)
        if timings is not None:
            t4 = time.perf_counter()
            timings.update(groups_s=t1 - t0, reports_s=t2 - t1, peaks_s=t3 - t2, clusters_s=t4 - t3)
        return tdir
    if n_groups:
        state = peaks(g, gaussian_table())
        res = peaks_results(off, state, device_rank=device_rank)
    else:
        res = []
    t3 = time.perf_counter()
    if n_groups:
        codes, nm, span, rpm, rows = g.codes, g.nmask, g.span, g.rpm, np.asarray(g.rows).reshape(-1, 3)
    group_sample = blocks[pairs[:, 0], 0] if n_groups else np.zeros(0, dtype=np.int32)
    for si, sample in enumerate(sampleList):
        def named(si=si):
            for k in np.nonzero(group_sample == si)[0].tolist():
                own, paired = int(pairs[k, 0]), int(pairs[k, 1])
                L = int(st.entries[blocks[own, 1], 1])
                yield (et.names[blocks[paired, 1]], ArrayGroup(codes, nm, span, rpm, rows, int(off[k]), int(off[k + 1]), L),
                       res[k])
        _write_clusters(tdir, sample, named(), stru, pretrnaNameSeqDic)
    if timings is not None:
        t4 = time.perf_counter()
        timings.update(groups_s=t1 - t0, reports_s=t2 - t1, peaks_s=t3 - t2, clusters_s=t4 - t3)
    return tdir
