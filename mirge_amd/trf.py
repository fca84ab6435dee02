"""tRF typing and tables for `-trf`.

Restates, on small host data:
  * the `-trf` table loading of __main__.py:164-251 (`load_trf_tables`);
  * `trfTypes` (runAnnotationPipeline.py:448-474) and the bookkeeping of
    `updatetrfContentDic2/3` (RAP:497-541) over the `-a --best --strata` listings that
    `parseAlignment3` (RAP:41-52) collects after the mature-tRNA pass (RAP:657-660) and the
    primary-tRNA-trailer pass (RAP:698-701);
  * the first part of writeDataToCSV's `if trf_output:` block (W2C:648-800):
    `tRFs.potential.report.tsv`, `discarded.reads.summary.assigningtRFs.csv`, `tRF.Counts.csv`,
    `tRF.RP100K.csv`, with `addDashNew`, `coordinate`, `getDistance2`, `assign_cluster`
    (W2C:353-392, :546-564).

The listings come from the GPU (`Engine.list_best` = mrg_list_best_count/fill); tests can pass
any `lister(reads, library_key, max_mismatches) -> [[(entry name, 0-based offset), ...], ...]`.

The command line runs the array route (entry_tables, row_order, raise_unresolved and sample_tables below +
mrg_trf_classify + mrg_write_trf_tables); the functions above them are its model and serve reads beyond 255 nt, a
`choose` other than min and `--trf-host`, as content_from_rows does for trf_samples.write_trf_samples.

The per-sample `tRFs.samples.tmp/*` reports and their density-peak clustering (W2C:802-1088), which
start from the trfContentDic that write_trf_tables leaves, are mirge_amd.trf_samples.

Where the reference is not deterministic it is pinned here:
  * `random.choice(candidatetRNAUniquelist)` (W2C:708) -> `choose`, default the
    lexicographically smallest name;
  * `list(set(...))` order of the de-duplicated hit columns (W2C:704) -> sorted.
"""
import os
import sys

from .isomir import NT2CODE, make_id


# ---------------------------------------------------------------- tables (MAIN:164-251)
def add_dash_new(seq, total_length, start, end):
    """W2C:353-355 (1-based inclusive start/end)."""
    return "-" * (start - 1) + seq + "-" * (total_length - end)


def load_trf_tables(library_path, species):
    """MAIN:164-251.  Returns a dict with trnaStruDic, trnaAAanticodonDic, duptRNA2UniqueDic,
    tRNAtrfDic, trfMergedNameDic, trfMergedList; a missing file prints the reference's message
    and exits 1."""
    ann = os.path.join(library_path, species, "annotation.Libs")

    def need(path):
        if not os.path.isfile(path):
            print("%s does not exsit. Please check it." % path, file=sys.stderr)
            sys.exit(1)
        return path

    stru = {}
    with open(need(os.path.join(ann, species + "_trna.str"))) as fh:
        line = fh.readline()
        while line != "":
            name = line.strip()[1:]
            seq = fh.readline().strip()
            st = fh.readline().strip()
            a = st.index("XXX") + 1          # 1-based
            stru[name] = {"seq": seq, "stru": st, "anticodonStart": a, "anticodonEnd": a + 2}
            line = fh.readline()
    aa = {}
    with open(need(os.path.join(ann, species + "_trna_aminoacid_anticodon.csv"))) as fh:
        for line in fh:
            f = line.strip().split(",")
            aa[f[0]] = {"aaType": f[1], "anticodon": f[2]}
    dup = {}
    with open(need(os.path.join(ann, species + "_trna_deduplicated_list.csv"))) as fh:
        fh.readline()
        for line in fh:
            if line == "":
                break
            f = line.strip().split(",")
            for item in f[1].split("/"):
                dup[item.strip()] = f[0].strip()
    clusters = {}
    with open(need(os.path.join(ann, species + "_tRF_infor.csv"))) as fh:
        fh.readline()
        for line in fh:
            f = line.strip().split(",")
            trna = f[0].split("_Cluster")[0]
            start, end = int(f[3].split("-")[0]), int(f[3].split("-")[1])
            clusters.setdefault(trna, {})[add_dash_new(f[4], len(f[5]), start, end)] = f[0]
    merged_name, merged_list = {}, []
    with open(need(os.path.join(ann, species + "_tRF_merges.csv"))) as fh:
        for line in fh:
            f = line.strip().split(",")
            merged_list.append(f[0])
            for item in f[1].split("/"):
                merged_name[item] = f[0]
    return {"trnaStruDic": stru, "trnaAAanticodonDic": aa, "duptRNA2UniqueDic": dup, "tRNAtrfDic": clusters,
            "trfMergedNameDic": merged_name, "trfMergedList": merged_list}


# ---------------------------------------------------------------- typing (RAP:448-541)
def trfTypes(seq, tRNAName, start, trnaStruDic, pretrnaNameSeqDic):
    """RAP:448-474; `start` 0-based."""
    if "pre_" in tRNAName:
        pretrnaNameSeqDic[tRNAName]          # the reference looks it up (KeyError if unknown)
        return "tRF-1"
    rec = trnaStruDic[tRNAName]
    n = len(rec["seq"])
    anticodon = rec["anticodonStart"] - 1
    last = start + len(seq) - 1
    if start == 0:
        if start + len(seq) == n:
            return "tRF-whole"
        if anticodon - 2 <= last <= anticodon + 1:
            return "5'-half"
        return "5'-tRF"
    if n - 3 <= last <= n - 1:
        if anticodon - 1 <= start <= anticodon + 2:
            return "3'-half"
        return "3'-tRF"
    return "i-tRF"


def update_trf_content_mature(trfContentDic, hits, trnaStruDic, pretrnaNameSeqDic, seqDic, sampleList):
    """updatetrfContentDic2 (RAP:497-516).  `hits` = {read: [(tRNA name, 0-based offset), ...]} in
    the order the SAM lists them (a later line for the same tRNA overwrites an earlier one)."""
    S = len(sampleList)
    for read, items in hits.items():
        rec = {"count": [int(seqDic[read]["quant"][i]) for i in range(S)], "uid": make_id(read, NT2CODE)}
        trfContentDic[read] = rec
        for name, start in items:
            rec[name] = {"tRFType": trfTypes(read, name, start, trnaStruDic, pretrnaNameSeqDic), "start": start,
                         "end": start + len(read) - 1, "cigar": "undifined"}


def update_trf_content_trailer(trfContentDic, hits, trnaStruDic, pretrnaNameSeqDic, seqDic, sampleList,
                               subseqSeqDic):
    """updatetrfContentDic3 (RAP:518-541).  `hits` is keyed by the T-stripped subsequence; every
    original read of subseqSeqDic[subsequence] gets the entry."""
    S = len(sampleList)
    for sub, items in hits.items():
        for read in subseqSeqDic[sub]:
            rec = {"count": [int(seqDic[read]["quant"][i]) for i in range(S)], "uid": make_id(read, NT2CODE)}
            trfContentDic[read] = rec
            tail_t = len(read) - len(read.rstrip("T"))
            for name, start in items:
                rec[name] = {"tRFType": trfTypes(read, name, start, trnaStruDic, pretrnaNameSeqDic),
                             "start": start, "end": start + len(read) - 1 - tail_t, "cigar": "undifined"}


def engine_lister(engine):
    """lister backed by the GPU: `-v V -a --best --strata --norc` against one library."""
    from . import pack
    from .engine import V_MODE_SEED, ReadSet

    def lister(reads, library_key, max_mismatches):
        if not reads:
            return []
        words, lens, nmask = pack.pack_reads(reads)
        rs = ReadSet(words, lens, nmask, None, device=engine.device)
        _, off, ref, pos = engine.list_best(rs, library_key, seed_len=V_MODE_SEED, max_mm_seed=max_mismatches,
                                            max_mm_total=max_mismatches)
        names = engine.indexes[library_key].names
        return [[(names[int(ref[k])], int(pos[k])) for k in range(int(off[i]), int(off[i + 1]))]
                for i in range(len(reads))]
    return lister


def strip_poly_t(read):
    """RAP:671-680: a read ending in >= 3 T, its T tail removed, if >= 11 nt remain; else None."""
    sub = read.rstrip("T")
    if len(read) - len(sub) >= 3 and len(sub) >= 11:
        return sub
    return None


def collect_trf_content(trfContentDic, seqDic, sampleList, trnaStruDic, pretrnaNameSeqDic, lister,
                        mature_key="mature_trna", pre_key="pre_trna"):
    """The `-trf` side products of the cascade (RAP:657-660, :698-701) after the cascade has set
    `annot`: reads claimed by pass 2 / pass 3 are listed against their library and typed.  Listings
    are consumed highest (entry, offset) first, so that for a tRNA hit twice by one read the lowest
    offset is kept -- the order in which the engine's tie rule would list them last."""
    mature = [s for s, r in seqDic.items() if r["annot"][3] != ""]
    lists = lister(mature, mature_key, 1)
    update_trf_content_mature(trfContentDic, {s: l[::-1] for s, l in zip(mature, lists)}, trnaStruDic,
                              pretrnaNameSeqDic, seqDic, sampleList)
    sub_reads = {}
    for s, r in seqDic.items():
        if r["annot"][4] != "":
            sub_reads.setdefault(strip_poly_t(s), []).append(s)
    subs = list(sub_reads)
    lists = lister(subs, pre_key, 0)
    update_trf_content_trailer(trfContentDic, {s: l[::-1] for s, l in zip(subs, lists)}, trnaStruDic,
                               pretrnaNameSeqDic, seqDic, sampleList, sub_reads)


# ---------------------------------------------------------------- tables (W2C:357-392, :546-564)
def coordinate(dashed):
    """W2C:357-371: 1-based first and last non-dash positions."""
    lead = len(dashed) - len(dashed.lstrip("-"))
    trail = len(dashed) - len(dashed.rstrip("-"))
    return lead + 1, len(dashed) - trail


def get_distance2(seq1, seq2):
    """W2C:373-392: |start shift| + |end shift| + substitutions (a base of seq1 past the end of
    seq2 counts as one: the reference's IndexError branch, reached only when seq1[k] is a base)."""
    c1, c2 = coordinate(seq1), coordinate(seq2)
    subst = 0
    for k in range(len(seq1)):
        if seq1[k] == "-":
            continue
        if k >= len(seq2) or (seq2[k] != "-" and seq1[k] != seq2[k]):
            subst += 1
    return abs(c1[0] - c2[0]) + abs(c1[1] - c2[1]) + subst


def assign_cluster(dashedSeq, tRNAName, tRNAtrfDic):
    """W2C:546-564."""
    if tRNAName not in tRNAtrfDic:
        return "Dele", 100, "Null"
    dis = sorted((get_distance2(dashedSeq, s), name) for s, name in tRNAtrfDic[tRNAName].items())
    if dis[0][0] <= 8.0:
        return dis[0][1], dis[0][0], dis[0][1]
    return "Undef", dis[0][0], dis[0][1]


def write_trf_tables(outputdir, sampleList, logDic, trfContentDic, tables, pretrnaNameSeqDic, choose=min):
    """W2C:648-800.  Mutates trfContentDic like the reference: adds 'RPM', keeps only the selected
    tRNA of every read, drops reads without a candidate."""
    stru, aa_dic = tables["trnaStruDic"], tables["trnaAAanticodonDic"]
    dup, clusters = tables["duptRNA2UniqueDic"], tables["tRNAtrfDic"]
    merged_name, merged_list = tables["trfMergedNameDic"], tables["trfMergedList"]
    S = len(sampleList)
    meta = ("uid", "RPM", "count")
    for rec in trfContentDic.values():
        rpm = []
        for i in range(S):
            q = logDic["quantStats"][i]
            denom = q["maturetrnaReads"] + q["pretrnaReads"]
            rpm.append(100000.0 * rec["count"][i] / denom if denom else 0.0)
        rec["RPM"] = rpm

    def info(read, name):
        e = trfContentDic[read][name]
        return ":".join([name, e["tRFType"], str(e["start"] + 1), str(e["end"] + 1)])

    def aa_of(name, type_from):
        t = aa_dic[type_from]["aaType"]
        return "pre:" + t if "pre_" in name else t

    rows = []
    trf_file = os.path.join(outputdir, "tRFs.potential.report.tsv")
    with open(trf_file, "w") as out:
        out.write("read sequence\tuid\tread count(%s)\tRP100K (%s)\tamino acid all hits\tamino acid-anticodon all "
                  "hits\ttRF information all hits\tamino acid all deduplicated hits\tamino acid-anticodon all "
                  "deduplicated hits\ttRF information all deduplicated hits\tamino acid one hit\tamino "
                  "acid-anticodon one hit\ttRF information one hit\n" % (",".join(sampleList), ",".join(sampleList)))
        for read in list(trfContentDic.keys()):
            rec = trfContentDic[read]
            infos, aa_anticodons, aa_types, candidates = [], [], [], []
            for name in rec:
                if name in meta:
                    continue
                infos.append(info(read, name))
                candidates.append(name)
                t = aa_of(name, name)
                if t not in ("Und", "pre:Und"):
                    pair = t + "-" + aa_dic[name]["anticodon"]
                    if pair not in aa_anticodons:
                        aa_anticodons.append(pair)
                    if t not in aa_types:
                        aa_types.append(t)
            unique = sorted(set(dup.get(c, c) for c in candidates))
            if not unique:
                del trfContentDic[read]
                continue
            selected = choose(unique)
            cols = [read, rec["uid"], ",".join(str(c) for c in rec["count"]),
                    ",".join("%.3f" % round(v, 3) for v in rec["RPM"]),
                    ",".join(aa_types), ",".join(aa_anticodons), ",".join(infos)]
            # W2C:727: the amino-acid type of every de-duplicated hit is read from the SELECTED tRNA
            d_types = [aa_of(t, selected) for t in unique]
            d_pairs = [a + "-" + aa_dic[t]["anticodon"] for a, t in zip(d_types, unique)]
            cols += [",".join(d_types), ",".join(d_pairs), ",".join(info(read, t) for t in unique)]
            one_type = aa_of(selected, selected)
            cols += [one_type, one_type + "-" + aa_dic[selected]["anticodon"], info(read, selected)]
            out.write("\t".join(cols) + "\n")
            rows.append((read, rec["count"], [float("%.3f" % round(v, 3)) for v in rec["RPM"]], selected,
                         rec[selected]["start"] + 1, rec[selected]["end"] + 1))
            for name in list(rec.keys()):
                if name not in meta and name != selected:
                    del rec[name]
    # W2C:749-800: counts per predefined tRF entity
    entity = {s: {m: [0, 0.0] for m in merged_list} for s in sampleList}
    summary = {s: [0, 0] for s in sampleList}
    for read, counts, rp100k, name, start, end in rows:
        length = len(pretrnaNameSeqDic[name]) if "pre" in name else len(stru[name]["seq"])
        assigned, _, _ = assign_cluster(add_dash_new(read, length, start, end), name, clusters)
        for i, s in enumerate(sampleList):
            summary[s][1] += counts[i]
            if assigned not in ("Undef", "Dele"):
                m = merged_name[assigned]
                entity[s][m][0] += counts[i]
                entity[s][m][1] += rp100k[i]
            else:
                summary[s][0] += counts[i]
    with open(os.path.join(outputdir, "discarded.reads.summary.assigningtRFs.csv"), "w") as out:
        out.write("sample name,percentage of discarded reads,details\n")
        for s in sampleList:
            d, t = summary[s]
            pct = round(float(d) / t * 100.0, 2) if t else 0.0
            out.write("%s,%.2f%%,%d\\%d\n" % (s, pct, d, t))
    with open(os.path.join(outputdir, "tRF.Counts.csv"), "w") as o1, \
            open(os.path.join(outputdir, "tRF.RP100K.csv"), "w") as o2:
        o1.write("entry name," + ",".join(sampleList) + "\n")
        o2.write("entry name," + ",".join(sampleList) + "\n")
        for m in merged_list:
            o1.write(m + "," + ",".join(str(entity[s][m][0]) for s in sampleList) + "\n")
            o2.write(m + "," + ",".join("%.2f" % round(entity[s][m][1], 2) for s in sampleList) + "\n")
    return rows


# ---------------------------------------------------------------------------------------------
# The array route of `-trf` (mrg_trf_classify + mrg_write_trf_tables, include/mirge_amd.h): what depends on the library
# entry alone is resolved once per entry here, with the expressions of the functions above; the per-read part runs on the
# GPU (csrc/trf_tables.hip) and the files are written by csrc/trf_tables_write.cpp.
TRF_TYPES = ("tRF-1", "tRF-whole", "5'-half", "5'-tRF", "3'-half", "3'-tRF", "i-tRF")
TYPE_UNRESOLVABLE, TYPE_RANGE = 7, 8
KIND_ASSIGNED, KIND_UNDEF, KIND_DELE, KIND_UNRESOLVABLE, KIND_RANGE, KIND_NONE = 0, 1, 2, 3, 4, 5
REC_INTS, HIT_INTS = 12, 4


class EntryTables:
    """entry_tables' result, over the entries of mature_trna followed by those of pre_trna (n_mature = the former).
    desc int32 [E, 8] = (template length or -1, len(stru seq), anticodonStart - 1, flags: 1 = "pre_" in name, 2 = trfTypes
    raises, rank of dup.get(name, name), entry of that name in the same library or -1, first and number of predefined tRFs);
    clusters int32 [T, 6] = (coordinate first, last, len(dashed), first word, rank of the cluster name, merged index or
    -1); words / plane uint64: the dashed strings, 2 bits per character (plane bit 2i = no ACGT: code 0 = N, 1 = another
    character; bit 2i + 1 = dash); names, rep_names, aa_types, anticodons per entry (None where trnaAAanticodonDic lacks the
    name); rep_aa_missing[e] = trnaAAanticodonDic lacks rep_names[e]; cluster_names, dashed per predefined tRF; merged_list;
    errors[(e, stage)] = the exception the Python route raises: stage "type" (trfTypes), "aa" (a hit without amino acid),
    "length" (the selected tRNA's template), and errors[("cluster", t)] (a predefined tRF without merged entity)."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def _pack_dashed(texts):
    """Dashed strings -> (words, plane, first word of each)."""
    import numpy as np
    lens = np.fromiter((len(t) for t in texts), dtype=np.int64, count=len(texts))
    first = np.zeros(len(texts) + 1, dtype=np.int64)
    np.cumsum((lens + 31) // 32, out=first[1:])
    total = int(first[-1])
    words = np.zeros(max(total, 1), dtype=np.uint64)
    plane = np.zeros(max(total, 1), dtype=np.uint64)
    if total:
        code = np.full(256, 5, dtype=np.uint8)
        for ch, v in (("A", 0), ("C", 1), ("G", 2), ("T", 3), ("N", 4), ("-", 6)):
            code[ord(ch)] = v
        c = code[np.frombuffer("".join(texts).encode("latin-1", "replace"), dtype=np.uint8)]
        base_off = np.zeros(len(texts) + 1, dtype=np.int64)
        np.cumsum(lens, out=base_off[1:])
        owner = np.repeat(np.arange(len(texts)), lens)
        i = np.arange(c.size) - base_off[owner]
        slot = first[owner] + (i >> 5)
        sh = ((i & 31) * 2).astype(np.uint64)
        value = np.where(c <= 3, c, np.where(c == 5, 1, 0)).astype(np.uint64)
        flag = np.where(c <= 3, 0, np.where(c == 6, 2, 1)).astype(np.uint64)
        np.bitwise_or.at(words, slot, value << sh)
        np.bitwise_or.at(plane, slot, flag << sh)
    return words, plane, first[:-1]


def entry_tables(mature_names, pre_names, tables, pre_seqs):
    """Per entry of the two tRNA libraries, everything collect_trf_content and write_trf_tables ask of an entry.  A lookup
    that raises there is kept per entry and raised only when a read reaches it (raise_unresolved)."""
    import numpy as np
    stru, aa_dic = tables["trnaStruDic"], tables["trnaAAanticodonDic"]
    dup, clusters_dic = tables["duptRNA2UniqueDic"], tables["tRNAtrfDic"]
    merged_name, merged_list = tables["trfMergedNameDic"], list(tables["trfMergedList"])
    names = list(mature_names) + list(pre_names)
    n_mature, E = len(mature_names), len(names)
    rep_names = [dup.get(x, x) for x in names]
    rank_of = {x: r for r, x in enumerate(sorted(set(rep_names)))}
    entry_of = ({}, {})
    for e in range(E - 1, -1, -1):
        entry_of[e >= n_mature][names[e]] = e
    merged_index = {}
    for g, x in enumerate(merged_list):
        merged_index.setdefault(x, g)
    cluster_rank = {x: r for r, x in enumerate(sorted({c for d in clusters_dic.values() for c in d.values()}))}
    desc = np.zeros((E, 8), dtype=np.int32)
    errors, aa_types, anticodons, rep_aa_missing = {}, [], [], np.zeros(E, dtype=bool)
    cluster_rows, cluster_names, dashed_all, slice_of = [], [], [], {}
    for e, name in enumerate(names):
        if "pre_" in name:
            desc[e, 3] |= 1
            if name not in pre_seqs:
                desc[e, 3] |= 2
                errors[(e, "type")] = KeyError(name)
        elif name in stru:
            desc[e, 1], desc[e, 2] = len(stru[name]["seq"]), stru[name]["anticodonStart"] - 1
        else:
            desc[e, 3] |= 2
            errors[(e, "type")] = KeyError(name)
        try:
            desc[e, 0] = len(pre_seqs[name]) if "pre" in name else len(stru[name]["seq"])
        except KeyError as err:
            desc[e, 0] = -1
            errors[(e, "length")] = err
        if name in aa_dic:
            aa_types.append(aa_dic[name]["aaType"])
            anticodons.append(aa_dic[name]["anticodon"])
        else:
            aa_types.append(None)
            anticodons.append(None)
            errors[(e, "aa")] = KeyError(name)
        desc[e, 4] = rank_of[rep_names[e]]
        desc[e, 5] = entry_of[e >= n_mature].get(rep_names[e], -1)
        rep_aa_missing[e] = rep_names[e] not in aa_dic
        if name not in slice_of:
            first = len(cluster_rows)
            for dashed, cname in clusters_dic.get(name, {}).items():
                c0, c1 = coordinate(dashed)
                t = len(cluster_rows)
                m = merged_index.get(merged_name[cname], -1) if cname in merged_name else -1
                if m < 0:
                    errors[("cluster", t)] = KeyError(cname)
                cluster_rows.append((c0, c1, len(dashed), 0, cluster_rank[cname], m))
                cluster_names.append(cname)
                dashed_all.append(dashed)
            slice_of[name] = (first, len(cluster_rows) - first)
        desc[e, 6], desc[e, 7] = slice_of[name]
    clusters = np.array(cluster_rows, dtype=np.int32).reshape(-1, 6)
    words, plane, first_word = _pack_dashed(dashed_all)
    if len(cluster_rows):
        clusters[:, 3] = first_word
    return EntryTables(desc=desc, clusters=clusters, words=words, plane=plane, names=names, rep_names=rep_names,
                       aa_types=aa_types, anticodons=anticodons, rep_aa_missing=rep_aa_missing, cluster_names=cluster_names,
                       dashed=dashed_all, merged_list=merged_list, errors=errors, n_mature=n_mature)


def row_order(rec, n_mature, words, lens, nmask=None):
    """The order of trfContentDic's keys, as a permutation of the rows of mrg_trf_classify: the rows of the mature pass as
    they are, then those of the trailer pass grouped by their T-stripped sequence -- groups in order of first appearance,
    rows inside a group in array order (update_trf_content_trailer walks subseqSeqDic).  No loop over reads."""
    import numpy as np
    rec = np.asarray(rec).reshape(-1, REC_INTS)
    k = rec.shape[0]
    order = np.arange(k, dtype=np.int64)
    t = rec[n_mature:]
    n3 = t.shape[0]
    if n3 < 2:
        return order
    idx = t[:, 0].astype(np.int64)
    sub = np.asarray(lens)[idx].astype(np.int64) - t[:, 10]
    cols = [sub]
    for w in range(np.asarray(words).shape[0]):
        nb = np.clip(sub - 32 * w, 0, 32)
        keep = np.where(nb >= 32, ~np.uint64(0), (np.uint64(1) << (2 * np.minimum(nb, 31)).astype(np.uint64)) - np.uint64(1))
        cols.append(np.asarray(words)[w, idx] & keep)
        if nmask is not None:
            cols.append(np.asarray(nmask)[w, idx] & keep)
    by_seq = np.lexsort(cols[::-1])
    new = np.zeros(n3, dtype=bool)
    for c in cols:
        new[1:] |= c[by_seq][1:] != c[by_seq][:-1]
    group = np.empty(n3, dtype=np.int64)
    group[by_seq] = np.cumsum(new)
    first = np.full(int(group.max()) + 1, n3, dtype=np.int64)
    np.minimum.at(first, group, np.arange(n3))
    order[n_mature:] = n_mature + np.lexsort((np.arange(n3), first[group]))
    return order


def raise_unresolved(et, rec, hits):
    """What the Python route does when a read reaches a name it cannot resolve: collect_trf_content's first exception, else
    the first of write_trf_tables' report loop, else the first of its counting loop.  rec in the order of the tsv."""
    import numpy as np
    rec = np.asarray(rec).reshape(-1, REC_INTS)
    hits = np.asarray(hits).reshape(-1, HIT_INTS)
    k = rec.shape[0]
    counts = rec[:, 9].astype(np.int64)
    row = np.repeat(np.arange(k), counts)                                   # the tsv row of every (row, hit) pair, and
    at = np.repeat(rec[:, 8].astype(np.int64) - np.cumsum(counts) + counts, counts) + np.arange(int(counts.sum()))   # its hit
    entry, typ = hits[at, 0], hits[at, 3]
    # collect_trf_content: a hit is typed before anything else looks at it (hits of a read from the highest entry down)
    bad_rows = np.union1d(row[typ >= TYPE_UNRESOLVABLE], np.nonzero(rec[:, 7] == KIND_RANGE)[0])
    if bad_rows.size:
        r = int(bad_rows[0])
        mine = row == r
        for e, ty in sorted(zip(entry[mine].tolist(), typ[mine].tolist()), reverse=True):
            if ty == TYPE_UNRESOLVABLE:
                raise et.errors[(e, "type")]
        raise IndexError("row %d: read %d: entry, offset or poly-T tail out of range" % (r, int(rec[r, 0])))
    # the report loop: a hit without amino acid, then a de-duplicated name that is no hit of the read or has no amino acid
    E = et.desc.shape[0]
    ok = entry < E
    entry = np.where(ok, entry, 0)
    no_aa = np.array([x is None for x in et.aa_types], dtype=bool)
    rep = et.desc[entry, 5].astype(np.int64)
    rep_is_hit = (rep >= 0) & np.isin(row * (E + 1) + rep, row * (E + 1) + entry)
    bad = no_aa[entry] | ~rep_is_hit | et.rep_aa_missing[entry]
    if bad.any():
        r = int(row[bad].min())
        mine = np.nonzero(row == r)[0]
        es = sorted(entry[mine].tolist(), reverse=True)
        for e in es:
            if no_aa[e]:
                raise et.errors[(e, "aa")]
        by_rank = sorted(set((int(et.desc[e, 4]), et.rep_names[e], bool(et.rep_aa_missing[e])) for e in es))
        for _, name, missing in by_rank:
            if missing:
                raise KeyError(name)
        have = {et.names[e] for e in es}
        for _, name, _ in by_rank:
            if name not in have:
                raise KeyError(name)
    # the counting loop: the selected tRNA's template, the merged entity of the assigned predefined tRF
    for r in np.nonzero((rec[:, 7] == KIND_UNRESOLVABLE) | (rec[:, 7] == KIND_ASSIGNED))[0].tolist():
        if rec[r, 7] == KIND_UNRESOLVABLE:
            raise et.errors.get((int(rec[r, 1]), "length"), KeyError("row %d" % r))
        if ("cluster", int(rec[r, 5])) in et.errors:
            raise et.errors[("cluster", int(rec[r, 5]))]


def content_from_rows(et, rec, seqs, quant, denom):
    """The trfContentDic write_trf_tables leaves (one tRNA per read, with uid, count and RPM), from the rows in the order of
    the tsv: what trf_samples.write_trf_samples starts from.  seqs[r] = the read of row r, quant[r] its counts, denom[s] =
    maturetrnaReads + pretrnaReads of sample s.  The per-read Python that remains on the array route."""
    content = {}
    S = len(denom)
    for r, row in enumerate(rec.tolist()):
        if row[7] > KIND_DELE:
            continue
        count = [int(x) for x in quant[r]]
        content[seqs[r]] = {"count": count, "uid": make_id(seqs[r], NT2CODE),
                            "RPM": [100000.0 * count[i] / denom[i] if denom[i] else 0.0 for i in range(S)],
                            et.names[row[1]]: {"tRFType": TRF_TYPES[row[4]], "start": row[2], "end": row[3],
                                               "cigar": "undifined"}}
    return content


class SampleTables:
    """sample_tables' result, over the entries of entry_tables: entries int32 [E, 4] = (rank of the entry's name among the
    distinct names in Python string order, template length or -1, flags: 1 = "pre_" in name, 2 = "pre" in name, 0); names =
    the distinct names in that order; templates per entry (None where the lookup raises), aa_types per entry (et's)."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def sample_tables(et, tables, pre_seqs):
    """Per entry, everything trf_samples.sample_trf_dic and sample_reports ask of an entry: the block it belongs to (entries
    of equal names are one block), its template (`pre_seqs[name]` if "pre" in name else `stru[name]["seq"]`: the two
    spellings "pre" / "pre_" stay two columns, as in entry_tables) and the amino acid of the summary."""
    import numpy as np
    stru = tables["trnaStruDic"]
    names = sorted(set(et.names))
    rank = {x: r for r, x in enumerate(names)}
    entries = np.zeros((len(et.names), 4), dtype=np.int32)
    templates = []
    for e, name in enumerate(et.names):
        try:
            t = pre_seqs[name] if "pre" in name else stru[name]["seq"]
        except KeyError:
            t = None
        templates.append(t)
        entries[e] = (rank[name], -1 if t is None else len(t), ("pre_" in name) | (("pre" in name) << 1), 0)
    return SampleTables(entries=entries, names=names, templates=templates, aa_types=list(et.aa_types), n_names=len(names))
