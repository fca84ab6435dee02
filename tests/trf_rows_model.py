"""The record and hit layout of mrg_trf_classify (include/mirge_amd.h), written down from the functions of
mirge_amd.trf: `rows` runs collect_trf_content (trfTypes, strip_poly_t), then the selection and
assign_cluster / add_dash_new / get_distance2 of write_trf_tables, and turns their results into the
rows the device call returns.  Shared by tests/test_trf_native.py (entry tables and the writer on the
CPU) and tests/test_gpu_trf_tables.py (the kernels)."""
import numpy as np

from mirge_amd import trf

META = ("uid", "RPM", "count")


def seq_dic(mature, trailer, quant=None):
    """A seqDic holding the given reads: annot slot 3 / 4 set as the cascade sets them."""
    out = {}
    for k, read in enumerate(list(mature) + list(trailer)):
        annot = [1] + [""] * 9
        annot[3 if k < len(mature) else 4] = "x"
        out[read] = {"annot": annot, "quant": [1] if quant is None else list(quant[k]), "length": len(read)}
    return out


def rows(et, tables, pre_seqs, mature, trailer, lister=None, index_of=None, content=None):
    """(rec int32 [k, 12], hits int32 [h, 4]) for the reads `mature` (pass 2) then `trailer` (pass 3), in that order;
    rec[:, 0] = index_of[read] (default: the row).  A trailer read strip_poly_t rejects is a row of kind "out of range".
    content: a trfContentDic collect_trf_content has built already (else it is built here with `lister`)."""
    stru = tables["trnaStruDic"]
    dup, clusters = tables["duptRNA2UniqueDic"], tables["tRNAtrfDic"]
    if content is None:
        listed = [r for r in trailer if trf.strip_poly_t(r) is not None]
        content = {}
        trf.collect_trf_content(content, seq_dic(mature, listed), ["s"], stru, pre_seqs, lister)
    rec = np.zeros((len(mature) + len(trailer), trf.REC_INTS), dtype=np.int32)
    hits = []
    for r, read in enumerate(list(mature) + list(trailer)):
        is_trailer = r >= len(mature)
        lo, hi = (et.n_mature, len(et.names)) if is_trailer else (0, et.n_mature)
        entry_of = {et.names[e]: e for e in range(hi - 1, lo - 1, -1)}
        rec[r, 0] = r if index_of is None else index_of[read]
        rec[r, 1], rec[r, 5], rec[r, 8] = -1, -1, len(hits)
        rec[r, 10] = len(read) - len(read.rstrip("T")) if is_trailer else 0
        if is_trailer and trf.strip_poly_t(read) is None:
            rec[r, 7], rec[r, 8] = trf.KIND_RANGE, 0
            continue
        c = content.get(read, {})
        names = [x for x in c if x not in META]
        if not names:
            rec[r, 7], rec[r, 8] = trf.KIND_NONE, 0
            continue
        for name in sorted(names, key=entry_of.get):
            h = c[name]
            hits.append((entry_of[name], h["start"], h["end"], trf.TRF_TYPES.index(h["tRFType"])))
        rec[r, 9] = len(names)
        selected = min(sorted(set(dup.get(x, x) for x in names)))
        if selected not in c:
            rec[r, 7] = trf.KIND_UNRESOLVABLE
            continue
        sel = c[selected]
        rec[r, 1], rec[r, 2], rec[r, 3] = entry_of[selected], sel["start"], sel["end"]
        rec[r, 4] = trf.TRF_TYPES.index(sel["tRFType"])
        try:
            length = len(pre_seqs[selected]) if "pre" in selected else len(stru[selected]["seq"])
        except KeyError:
            rec[r, 7] = trf.KIND_UNRESOLVABLE
            continue
        dashed = trf.add_dash_new(read, length, sel["start"] + 1, sel["end"] + 1)
        assigned, dist, nearest = trf.assign_cluster(dashed, selected, clusters)
        rec[r, 6] = dist
        if assigned == "Dele":
            rec[r, 7] = trf.KIND_DELE
            continue
        rec[r, 7] = trf.KIND_UNDEF if assigned == "Undef" else trf.KIND_ASSIGNED
        first, count = int(et.desc[entry_of[selected], 6]), int(et.desc[entry_of[selected], 7])
        rec[r, 5] = next(t for t in range(first, first + count)
                         if et.cluster_names[t] == nearest and trf.get_distance2(dashed, et.dashed[t]) == dist)
    return rec, np.array(hits, dtype=np.int32).reshape(-1, trf.HIT_INTS)


def cluster_key(et, rec):
    """(kind, distance, nearest cluster NAME) per row: two predefined strings of one tRNA may carry one name."""
    return [(int(k), int(d), et.cluster_names[c] if c >= 0 else None) for k, d, c in rec[:, [7, 6, 5]].tolist()]


def brute_lister(libs):
    """`-v V -a --best --strata --norc` by exhaustive comparison: libs[key] = (names, seqs).  A read's N differs from
    everything.  -> lister(reads, key, v) as trf.collect_trf_content takes it, listings sorted by (entry, offset)."""
    arrays = {key: [np.frombuffer(s.encode(), dtype=np.uint8) for s in seqs] for key, (_, seqs) in libs.items()}

    def lister(reads, key, v):
        names = libs[key][0]
        out = []
        for read in reads:
            r = np.frombuffer(read.encode(), dtype=np.uint8).copy()
            r[r == ord("N")] = 0
            found, best = [], v
            for e, seq in enumerate(arrays[key]):
                if len(seq) < len(r) or not len(r):
                    continue
                mm = (np.lib.stride_tricks.sliding_window_view(seq, len(r)) != r).sum(axis=1)
                low = int(mm.min())
                if low > best:
                    continue
                if low < best:
                    found, best = [], low
                found += [(names[e], int(at)) for at in np.nonzero(mm == low)[0]]
            out.append(found)
        return out
    return lister
