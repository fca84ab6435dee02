"""Predict mode's genome mapping and location clustering in one call (reference miRge2.0.py:538-548): the alignments of
the `-f -n 0 -m <mapping_loc> -l <seedLength> -a --best` genome run never become SAM text on their way to the cluster
table.  They stay on the GPU as rows, are sorted by coordinate there and merged by cluster_basedon_location.py's rule
(Engine.cluster_valid = mrg_list_valid_count / _fill, mrg_cluster_keys / _sort / _scan / _bounds / _assemble); the host
writers (mrg_write_clusters, mrg_write_sorted_sam) print

    <out_stem>_vs_genome_sorted_clusters.tsv    byte for byte the reference's table
    <out_stem>_vs_genome_sorted.sam             the coordinate-sorted SAM that decorateSam (miRge2.0.py:596) reads

so the samtools view / sort / index / view round trip of this stage is gone.  Rows of the sorted SAM are ordered by
(entry, position, + before -, read order); unaligned and `-m`-suppressed reads follow in input order.  The order among
alignments with equal (entry, strand, position) is read order: a choice, not pinned against a real `samtools sort`.

    python -m mirge_amd.predict clusters <genome_prefix> <reads.fa> -m 3 -l 25 --overlap 14 -o <out_stem> [--no-sam]
                                         [--trim [--repeats FILE] [-clc 30] [--remap [--features]]]

With `trim=(repeats, cutoff)` / `--trim` the next two calls of the reference (preTrimClusteredSeq, generate_Seq; miRge2.0.py:557-562)
run over the same device arrays (Engine.predict_trim = mrg_predict_trim; mrg_write_trimmed_clusters) and add

    <out_stem>_vs_genome_sorted_clusters_trimmed.tsv        OriginalSeq, Flag and repetitiveElementName in front of every row
    <out_stem>_vs_genome_sorted_clusters_trimmed.fa         the retained clusters' sequences
    <out_stem>_vs_genome_sorted_clusters_trimmed_orig.fa    ... and their OriginalSeq

The repeat elements come from a four-column tab-separated file (load_repeats), not from the reference's pickle.

With `remap=True` / `--remap` (needs the trim) the block after that (miRge2.0.py:566-601: bowtie-build over the retained
clusters, two bowtie passes of the same reads, utils/processSam.py, `sort -k6,6 -k1,1`) runs over the same arrays
(map_reads_to_clusters: Engine.predict_remap = mrg_predict_trim_reads / mrg_predict_remap_rows; mrg_write_remapped_rows) and adds

    <out_stem>_vs_representative_seq_modified_selected_sorted.tsv    the only file generate_featureFiles reads

With `features=True` / `--features` (needs the remap) the call after that (miRge2.0.py:604, generate_featureFiles) runs over the
rows the remap left on the device (cluster_features: Engine.predict_features = mrg_predict_feature_groups / _align / _tally /
_neighbors; mrg_write_predict_features) and adds

    <out_stem>_vs_representative_seq_modified_selected_sorted_features.tsv    one line per cluster with a stable stretch
    <out_stem>_vs_representative_seq_modified_selected_sorted_cluster.txt     the aligned members of every cluster that got that far

With `classify=True, models=<dir>, species=...` / `--classify --models DIR [-sp SPECIES]` (needs the screening: `screen=True,
fold=...` / `--screen`) the last two calls before the report (miRge2.0.py:647-648, preprocess_featureFiles and model_predict) run
over the screened table (classify_candidates: the native reader and writers of ScreenedTable, Engine.predict_svm =
mrg_predict_svm; the model file read by mirge_amd/svm_model.py, before any device work) and add, next to the table,

    <tmp>.csv, <tmp>_refined_tmp.csv, <tmp>_refined_features.csv    the three filter files, <tmp> = ..._vs_dataset_15
    predicted_<sample>_detailed.csv                                   label and probability of every refined row
    <sample>_novel_miRNAs_miRge2.0.csv                                the rows predicted 1 with a probability of 0.8 or more

With `report=True` / `--report` (needs the classification) the last call (miRge2.0.py:652, write_novel_report) runs over the novel
list, the screened table and `_cluster.txt` (report_candidates: the native reader ReportInputs, Engine.predict_report =
mrg_predict_report_correct / _entries / _profile, the native writers) and adds

    <table>_corrected.tsv                              the screened table after the pair correction and the arm re-type
    <sample>_novel_miRNAs_report.csv                   one line per novel miRNA, byte for byte the reference's
    <sample>_novel_miRNAs_report_profiles.tsv          extension: per miRNA the padded read rows and the per-position coverage

Only the drawing of write_novel_report is left out: precusorTmp.fa / .str, the RNAfold run per miRNA and the PDFs are not made.

The device is $MIRGE_AMD_GPU (default 0).  Limits: reads up to 255 nt, fewer than 2^32 - 1 alignment rows, positions
below 2^31; beyond them the call fails naming the limit and writes nothing.
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

from . import bowtie, pack
from ._native import MirgeAmdError

HEADER = "miRClusterID\tChr\tStrand\tStart\tEnd\tSequence\tSequenceLenght\tCoutOfReads\tCountOfMembers\tMembers\n"


def sample_name(sam_path):
    """The reference's sample name: the file's base name minus its last three `_`-separated fields."""
    return "_".join(os.path.basename(sam_path).split("_")[:-3])


def _ptr(a):
    return a.ctypes.data if a.size else None


def read_counts(names):
    """counts[r] = the integer after the first `_` of read r's name (`mir<k>_<count>`); ValueError without one."""
    from . import _native
    lib = _native.load()
    nb, no = bowtie._blob(names)
    counts = np.zeros(len(names), dtype=np.uint32)
    bad = C.c_int64(-1)
    rc = lib.mrg_read_counts_from_names(len(names), nb, no.ctypes.data, _ptr(counts), C.byref(bad))
    if rc != 0:
        if bad.value >= 0:
            raise ValueError("read name %r has no `_<count>` field below 2^32" % names[bad.value])
        _native.check(rc)
    return counts


def _blob(strs):
    """(blob, offsets uint64 [n + 1], n) of a list of strings, or of a ready (blob, offsets) pair (mrg_predict_read_names,
    pack.unpack_blob), which is passed through."""
    if isinstance(strs, tuple) and len(strs) == 2 and isinstance(strs[0], (bytes, bytearray, memoryview, np.ndarray)):
        blob, off = strs
        off = np.ascontiguousarray(off, dtype=np.uint64)
        return (blob if isinstance(blob, bytes) else bytes(blob)), off, int(off.shape[0]) - 1
    blob, off = bowtie._blob(strs)
    return blob, off, len(strs)


def read_names(numbers, counts):
    """The names `mir<number>_<count>` of a list's rows as one blob plus offsets (mrg_predict_read_names): the pair
    write_clusters and write_sorted_sam take in place of a list of names.  counts: uint32 or uint64."""
    from . import _native
    lib = _native.load()
    numbers = np.ascontiguousarray(numbers, dtype=np.uint32)
    counts = np.ascontiguousarray(counts)
    if counts.dtype != np.uint64:
        counts = np.ascontiguousarray(counts, dtype=np.uint32)
    k = int(numbers.shape[0])
    if counts.shape != (k,):
        raise ValueError("read_names: one count per number")
    off = np.zeros(k + 1, dtype=np.uint64)
    need = C.c_uint64(0)
    _native.check(lib.mrg_predict_read_names(_ptr(numbers), _ptr(counts), counts.dtype.itemsize, k, None, 0, off.ctypes.data,
                                             C.byref(need)))
    blob = np.zeros(max(int(need.value), 1), dtype=np.uint8)
    _native.check(lib.mrg_predict_read_names(_ptr(numbers), _ptr(counts), counts.dtype.itemsize, k, blob.ctypes.data,
                                             int(need.value), off.ctypes.data, C.byref(need)))
    return blob[:int(need.value)].tobytes(), off


def write_clusters(path, sample, parts, names, cl, threads=None):
    """mrg_write_clusters over the arrays of Engine.cluster_valid (parts: the FmIndex list; names: the reads', a list or
    the (blob, offsets) pair of read_names)."""
    from . import _native
    lib = _native.load()
    nb, no, n_reads = _blob(names)
    hs = (C.c_void_p * max(len(parts), 1))(*[p._h.value for p in parts])
    arr = {k: np.ascontiguousarray(cl[k], dtype=dt) for k, dt in
           (("entry", np.uint32), ("strand", np.uint8), ("start", np.uint32), ("end", np.uint32), ("seq_off", np.uint64),
            ("count_sum", np.uint64), ("member_off", np.uint32), ("members", np.uint32))}
    seq = np.frombuffer(bytes(cl["seq"]), dtype=np.uint8)
    rows = C.c_uint64()
    with _writer_threads(threads):
        _native.check(lib.mrg_write_clusters(
            os.fsencode(path), sample.encode(), hs, len(parts), len(arr["entry"]), _ptr(arr["entry"]), _ptr(arr["strand"]),
            _ptr(arr["start"]), _ptr(arr["end"]), arr["seq_off"].ctypes.data, _ptr(seq), _ptr(arr["count_sum"]),
            arr["member_off"].ctypes.data, _ptr(arr["members"]), n_reads, nb, no.ctypes.data, C.byref(rows)))
    return int(rows.value)


def write_sorted_sam(path, parts, names, seqs, rows, suppressed, m, threads=None):
    """mrg_write_sorted_sam: rows = (read, entry, offset, strand, mm) in the order to print.  names / seqs: lists, or
    (blob, offsets) pairs (read_names, pack.unpack_blob)."""
    from . import _native
    lib = _native.load()
    nb, no, n_reads = _blob(names)
    sb, so, n_seqs = _blob(seqs)
    if n_seqs != n_reads:
        raise ValueError("write_sorted_sam: %d names and %d sequences" % (n_reads, n_seqs))
    hs = (C.c_void_p * max(len(parts), 1))(*[p._h.value for p in parts])
    read, entry, offset, strand, mm = (np.ascontiguousarray(a, dtype=dt) for a, dt in
                                       zip(rows, (np.uint32, np.int32, np.int32, np.uint8, np.uint8)))
    supp = np.ascontiguousarray(suppressed, dtype=np.uint8)
    summary = np.zeros(4, dtype=np.uint64)
    with _writer_threads(threads):
        _native.check(lib.mrg_write_sorted_sam(
            os.fsencode(path), hs, len(parts), n_reads, nb, no.ctypes.data, sb, so.ctypes.data, len(read), _ptr(read),
            _ptr(entry), _ptr(offset), _ptr(strand), _ptr(mm), _ptr(supp), int(m), summary.ctypes.data))
    return dict(processed=int(summary[0]), aligned=int(summary[1]), suppressed=int(summary[2]), reported=int(summary[3]))


def repeats_path(lib, species):
    """Where `annotate --novel-trim` looks for the repeat elements of a species."""
    return os.path.join(lib, species, "annotation.Libs", "%s_genome_repeats.tsv" % species)


def load_repeats(path, parts):
    """The repeat elements of a genome as flat arrays.  path: a tab-separated file of `chr  start  end  name` lines (1-based
    inclusive coordinates; lines starting with `#` and a first line `chr start end name` are skipped); None or a missing file
    is an empty table, as the reference's IOError branch leaves every chromosome without one.  parts: the genome's FmIndex
    list, whose entry names are the chromosomes; rows of a chromosome the genome lacks are dropped.
    Returns a dict: rep_off (uint32 [entries + 1]: entry e owns elements rep_off[e] .. rep_off[e + 1]), start, end, name_id
    (uint32 per element, sorted stably by start inside an entry), names (list), names_blob / names_off (uint64), parts."""
    entries = [nm for ix in parts for nm in ix.names]
    number = {}
    for i, nm in enumerate(entries):
        number.setdefault(nm, i)
    ent, start, end, name_id, names, ids = [], [], [], [], [], {}
    lines = []
    if path is not None and os.path.isfile(path):
        with open(path) as fh:
            lines = fh.read().split("\n")
    for ln, line in enumerate(lines, 1):
        if not line or line.startswith("#"):
            continue
        f = line.rstrip("\r").split("\t")
        if ln == 1 and f == ["chr", "start", "end", "name"]:
            continue
        try:
            if len(f) != 4:
                raise ValueError
            s0, e0 = int(f[1]), int(f[2])
            if not (0 <= s0 < 2 ** 32 and 0 <= e0 < 2 ** 32):
                raise ValueError
        except ValueError:
            raise ValueError("%s line %d: expected `chr<TAB>start<TAB>end<TAB>name` with coordinates in [0, 2^32)" % (path, ln))
        e = number.get(f[0])
        if e is None:
            continue
        k = ids.get(f[3])
        if k is None:
            k = ids[f[3]] = len(names)
            names.append(f[3])
        ent.append(e)
        start.append(s0)
        end.append(e0)
        name_id.append(k)
    ent, start = np.array(ent, dtype=np.int64), np.array(start, dtype=np.uint32)
    order = np.lexsort((start, ent))          # (stable: rows of one entry and start keep the file's order)
    rep_off = np.zeros(len(entries) + 1, dtype=np.uint32)
    np.cumsum(np.bincount(ent, minlength=len(entries)), out=rep_off[1:])
    nb, no = bowtie._blob(names)
    return dict(rep_off=rep_off, start=start[order], end=np.array(end, dtype=np.uint32)[order],
                name_id=np.array(name_id, dtype=np.uint32)[order], names=names, names_blob=nb, names_off=no, parts=parts)


def write_trimmed_clusters(stem, sample, names, cl, trimmed, repeats, threads=None):
    """mrg_write_trimmed_clusters: `<stem>_trimmed.tsv`, `<stem>_trimmed.fa` and `<stem>_trimmed_orig.fa` from the arrays of
    Engine.cluster_valid (cl), Engine.predict_trim (trimmed: flag, rep, orig) and load_repeats.  Returns (rows, retained)."""
    from . import _native
    lib = _native.load()
    parts = repeats["parts"]
    nb, no, n_reads = _blob(names)
    hs = (C.c_void_p * max(len(parts), 1))(*[p._h.value for p in parts])
    arr = {k: np.ascontiguousarray(cl[k], dtype=dt) for k, dt in
           (("entry", np.uint32), ("strand", np.uint8), ("start", np.uint32), ("end", np.uint32), ("seq_off", np.uint64),
            ("count_sum", np.uint64), ("member_off", np.uint32), ("members", np.uint32))}
    K = len(arr["entry"])
    seq = np.frombuffer(bytes(cl["seq"]), dtype=np.uint8)
    orig = np.frombuffer(bytes(trimmed["orig"]), dtype=np.uint8)
    flag = np.ascontiguousarray(trimmed["flag"], dtype=np.uint8)
    rep = np.ascontiguousarray(trimmed["rep"], dtype=np.int32)
    if flag.shape != (K,) or rep.shape != (K,) or orig.shape != seq.shape or arr["seq_off"].shape != (K + 1,) or \
            int(arr["seq_off"][-1]) != seq.shape[0]:
        raise ValueError("write_trimmed_clusters: flag and rep [K], orig and seq [seq_off[K]] must match the clusters")
    name_id = np.ascontiguousarray(repeats["name_id"], dtype=np.uint32)
    rn_off = np.ascontiguousarray(repeats["names_off"], dtype=np.uint64)
    rows, kept = C.c_uint64(), C.c_uint64()
    with _writer_threads(threads):
        _native.check(lib.mrg_write_trimmed_clusters(
            os.fsencode(stem + "_trimmed.tsv"), os.fsencode(stem + "_trimmed.fa"), os.fsencode(stem + "_trimmed_orig.fa"),
            sample.encode(), hs, len(parts), K, _ptr(arr["entry"]), _ptr(arr["strand"]), _ptr(arr["start"]), _ptr(arr["end"]),
            arr["seq_off"].ctypes.data, _ptr(seq), _ptr(arr["count_sum"]), arr["member_off"].ctypes.data, _ptr(arr["members"]),
            n_reads, nb, no.ctypes.data, _ptr(flag), _ptr(rep), _ptr(orig), len(name_id), _ptr(name_id), len(rn_off) - 1,
            repeats["names_blob"], rn_off.ctypes.data, C.byref(rows), C.byref(kept)))
    return int(rows.value), int(kept.value)


def trim_clusters(engine, cl, repeats, clusterSeqLenCutoff, out_stem, names, threads=None, timings=None):
    """The reference's miRge2.0.py:557-562 over the clusters of Engine.cluster_valid (cl; with keep_device=True its arrays
    are taken where they are, else uploaded): preTrimClusteredSeq(repeats, <out_stem>_vs_genome_sorted_clusters.tsv,
    clusterSeqLenCutoff) and generate_Seq.  Writes `<out_stem>_vs_genome_sorted_clusters_trimmed.tsv`, `..._trimmed.fa` and
    `..._trimmed_orig.fa`; returns Engine.predict_trim's dict (flag, rep, orig and the retained arrays) plus n_retained.
    repeats: load_repeats' dict over the genome's parts; names: the reads' as write_clusters takes them.  timings gets
    trim_ms / download_ms (device events) and write_s."""
    import time
    cutoff = int(clusterSeqLenCutoff)
    if cutoff < 0:
        raise ValueError("clusterSeqLenCutoff must not be negative")
    t = engine.predict_trim(cl.get("device") or cl, repeats, cutoff, timings=timings)
    sam_path = out_stem + "_vs_genome_sorted.sam"
    t0 = time.perf_counter()
    _, t["n_retained"] = write_trimmed_clusters(sam_path[:-4] + "_clusters", sample_name(sam_path), names, cl, t, repeats, threads)
    if timings is not None:
        timings["write_s"] = time.perf_counter() - t0
    return t


REMAP_SUFFIX = "_vs_representative_seq_modified_selected_sorted.tsv"
REMAP_TRIMS = (1, 3)      # the second pass's -5 1 -3 3


def write_remapped_rows(path, words, lens, nmask, numbers, counts, index, kept_seq_off, kept_orig, rows, trims=REMAP_TRIMS,
                        threads=None):
    """mrg_write_remapped_rows: the sorted table of the second mapping from host arrays -- the packed reads (words uint64
    [W, n], lens, nmask or None), their numbers and counts (uint32 [n]), the cluster library (an FmIndex whose entry j is
    retained cluster j), kept_seq_off / kept_orig of Engine.predict_trim and rows = (read, cluster, offset, mm, pass) of
    Engine.predict_remap.  Returns the lines written."""
    from . import _native
    lib = _native.load()
    words = np.ascontiguousarray(words, dtype=np.uint64)
    if words.ndim != 2:
        raise ValueError("write_remapped_rows: words must be [W, n]")
    W, n = words.shape
    lens = np.ascontiguousarray(lens, dtype=np.uint8)
    nm = None if nmask is None else np.ascontiguousarray(nmask, dtype=np.uint64)
    numbers, counts = np.ascontiguousarray(numbers, dtype=np.uint32), np.ascontiguousarray(counts, dtype=np.uint32)
    soff = np.ascontiguousarray(kept_seq_off, dtype=np.uint64)
    orig = np.frombuffer(bytes(kept_orig), dtype=np.uint8)
    read, cluster, offset = (np.ascontiguousarray(a, dtype=np.uint32) for a in rows[:3])
    mm, pass_ = (np.ascontiguousarray(a, dtype=np.uint8) for a in rows[3:5])
    K = int(soff.shape[0]) - 1
    if lens.shape != (n,) or numbers.shape != (n,) or counts.shape != (n,) or (nm is not None and nm.shape != words.shape):
        raise ValueError("write_remapped_rows: words [W, n], nmask, lens, numbers and counts [n] must match")
    if K < 0 or int(soff[-1]) != orig.shape[0] or (index.n_ref if index is not None else 0) != K:
        raise ValueError("write_remapped_rows: kept_seq_off [K + 1] must close at the bytes of kept_orig and the library hold K entries")
    if any(a.shape != read.shape for a in (cluster, offset, mm, pass_)):
        raise ValueError("write_remapped_rows: the row arrays differ in length")
    done = C.c_uint64()
    with _writer_threads(threads):
        _native.check(lib.mrg_write_remapped_rows(
            os.fsencode(path), _ptr(words), W, n, _ptr(lens), None if nm is None else _ptr(nm), n, _ptr(numbers), _ptr(counts),
            index._h if index is not None else None, K, soff.ctypes.data, _ptr(orig), len(read), _ptr(read), _ptr(cluster),
            _ptr(offset), _ptr(mm), _ptr(pass_), int(trims[0]), int(trims[1]), C.byref(done)))
    return int(done.value)


def read_numbers(names):
    """numbers[r] = the n of read r's name `mir<n>_<count>`; ValueError without one below 2^32."""
    out = np.zeros(len(names), dtype=np.uint32)
    for r, nm in enumerate(names):
        head = nm[3:].split("_")[0] if nm.startswith("mir") else ""
        if not head.isdigit() or int(head) >= 2 ** 32:
            raise ValueError("read name %r is not `mir<n>_<count>` with n below 2^32" % nm)
        out[r] = int(head)
    return out


def map_reads_to_clusters(engine, rs, numbers, counts, trim_result, seedLength, out_stem, names=None, threads=None, timings=None,
                          keep_device=False):
    """The reference's miRge2.0.py:566-601 from the arrays: the sample's filtered reads (rs: the ReadSet the genome stage
    listed; numbers / counts [n]: their `mir<number>_<count>`, host arrays or device tensors; numbers None = read from
    `names`, a list) against the clusters trim_clusters retained (trim_result: its return value), in two passes -- bowtie's
    `-n 0 -l seedLength -a --best --norc`, then `-n 1 -l 15 -5 1 -3 3 -a --best --strata --norc` for the reads the first left
    unaligned -- decorated, selected and sorted as `LC_ALL=C sort -k6,6 -k1,1` does.  Writes
    `<out_stem>_vs_representative_seq_modified_selected_sorted.tsv`; returns a dict: rows (read, cluster, offset, mm, pass:
    host arrays in file order), n_rows, aligned1, aligned2, unaligned (reads).
    The cluster library is built on the device from `<out_stem>_vs_genome_sorted_clusters_trimmed_orig.fa`, the file the
    trim wrote, and is resident on an engine of its own for the duration of the call: engine.libs is untouched.  With no
    retained cluster nothing is written and every count is 0 (the reference aborts there).
    keep_device=True leaves the rows on the device too ("device": the tensors of Engine.predict_remap) and adds "index", the
    cluster library, for cluster_features."""
    import time
    import torch
    from .engine import Engine
    from .index import FmIndex
    if int(seedLength) < 5:
        raise ValueError("seedLength must be >= 5")
    empty = dict(rows=(np.zeros(0, np.uint32), np.zeros(0, np.uint32), np.zeros(0, np.uint32), np.zeros(0, np.uint8), np.zeros(0, np.uint8)),
                 n_rows=0, aligned1=0, aligned2=0, unaligned=0)
    K = int(trim_result["n_retained"]) if "n_retained" in trim_result else len(trim_result["kept"])
    if K == 0:
        return empty
    if K != len(trim_result["kept"]) or len(trim_result["kept_seq_off"]) != K + 1:
        raise ValueError("map_reads_to_clusters: the trim result's kept arrays contradict its retained count")

    def host_u32(x):
        return np.ascontiguousarray(x.cpu().numpy()).view(np.uint32) if torch.is_tensor(x) else np.ascontiguousarray(x, dtype=np.uint32)
    if numbers is None:
        numbers = read_numbers(names)
    n = 0 if rs is None else rs.n
    numbers, counts = host_u32(numbers), host_u32(counts)
    if numbers.shape != (n,) or counts.shape != (n,):
        raise ValueError("map_reads_to_clusters: numbers and counts must hold one value per read")
    path = out_stem + REMAP_SUFFIX
    index = FmIndex.from_fasta(out_stem + "_vs_genome_sorted_clusters_trimmed_orig.fa", device=engine.device_index)
    if index.n_ref != K:
        raise ValueError("map_reads_to_clusters: %d records in the clusters' FASTA, %d retained clusters" % (index.n_ref, K))
    if n == 0:
        write_remapped_rows(path, np.zeros((1, 0), np.uint64), np.zeros(0, np.uint8), None, numbers, counts, index,
                            trim_result["kept_seq_off"], trim_result["kept_orig"], empty["rows"], threads=threads)
        return empty
    scratch = Engine(engine.device_index)
    try:
        scratch.add_library("clusters", index, exact_dict=False)
        got = scratch.predict_remap(rs, numbers, "clusters", trim_result["kept"], int(seedLength), REMAP_TRIMS, timings=timings)
    finally:
        scratch.close()
    if keep_device:
        got["index"] = index
    else:
        got.pop("device", None)
    t0 = time.perf_counter()
    write_remapped_rows(path, rs.words.cpu().numpy().view(np.uint64), rs.lens.cpu().numpy(),
                        None if rs.nmask is None else rs.nmask.cpu().numpy().view(np.uint64), numbers, counts, index,
                        trim_result["kept_seq_off"], trim_result["kept_orig"], got["rows"], threads=threads)
    if timings is not None:
        timings["write_s"] = time.perf_counter() - t0
    return got


FEATURES_SUFFIX, CLUSTER_SUFFIX = "_features.tsv", "_cluster.txt"


def retained_clusters(cl, trim_result):
    """entry, strand, start, end of the clusters the trim retained (host arrays [K]), from Engine.cluster_valid's arrays."""
    kept = np.ascontiguousarray(trim_result["kept"], dtype=np.uint32).astype(np.int64)
    return {k: np.ascontiguousarray(np.asarray(cl[k])[kept], dtype=dt)
            for k, dt in (("entry", np.uint32), ("strand", np.uint8), ("start", np.uint32), ("end", np.uint32))}


def ratio_reached(c, total):
    """float(c) / total >= 0.8 as the reference asks it, decided in integers."""
    return 5 * int(c) >= 4 * int(total)


def host_group(cseq, seqs, counts):
    """One group of the feature table worked out on the host, for the groups the device leaves (a read or cluster beyond
    32 nt, an N, a gapped or unsettled alignment): a2i.local_pair per member, the frame, the column tallies and the nine
    feature columns' counts.  Returns (rows, numbers): rows = the cluster's padded row and every member's; numbers = None
    without a stable column, else a dict of H, T, head, tail, exact and nine [45] as mrg_predict_feature_tally leaves them."""
    from .a2i import local_pair
    rows, exact = [], 0
    for seq, count in zip(seqs, counts):
        cpad, spad = local_pair(cseq, seq)
        if sum(1 for x, y in zip(cpad, spad) if x == y and x != "-") == len(seq):
            exact += int(count)
        if not rows:
            rows = [cpad, spad]
        elif cpad == rows[0]:
            rows.append(spad)
        else:
            h1, h2 = cpad.index(cseq), rows[0].index(cseq)
            dh, dt = h1 - h2, (len(cpad) - h1) - (len(rows[0]) - h2)
            if dh > 0 or dt > 0:
                rows = ["-" * max(dh, 0) + r + "-" * max(dt, 0) for r in rows]
            rows.append("-" * max(-dh, 0) + spad + "-" * max(-dt, 0))
    width, total = len(rows[0]), sum(int(c) for c in counts)

    def tally(x):   # A, T, C, G, dash of column x; a column outside the frame is padding
        t = [0, 0, 0, 0, 0]
        for row, count in zip(rows[1:], counts):
            t["ATCG".find(row[x]) if 0 <= x < width else 4] += int(count)
        return t
    stable = [ratio_reached(max(tally(x)[:4]), total) for x in range(width)]
    if not any(stable):
        return rows, None
    head = stable.index(True)
    tail = (width - 1 - stable[::-1].index(True)) - width
    pad_t = max(0, 6 + tail + 1)
    tp = tail if pad_t == 0 else -6
    cols = [head - 3 + k for k in range(3)] + [width + pad_t + tp + k for k in range(6)]
    nine = [v for x in cols for v in tally(x)]
    H, T = len(rows[0]) - len(rows[0].lstrip("-")), len(rows[0]) - len(rows[0].rstrip("-"))
    return rows, dict(H=H, T=T, head=head, tail=tail, exact=exact, nine=nine)


def write_predict_features(table_path, parts, index, clusters, kept_seq_off, kept_orig, words, lens, nmask, counts, res, group_text=None,
                           threads=None):
    """mrg_write_predict_features: `<table>_features.tsv` and `<table>_cluster.txt` next to the table `table_path` names,
    from host arrays -- the genome's parts, the cluster library, the retained clusters (entry, strand, start, end;
    kept_seq_off, kept_orig), the packed reads with their counts, and res = the dict of Engine.predict_features with
    row_read added.  group_text: {group: text} for the groups the host worked out.  Returns (cluster blocks, feature lines)."""
    from . import _native
    lib = _native.load()
    base = os.path.basename(table_path).split("_")
    if base[0] == "mapped" and len(base) > 1 and base[1] == "mirna":
        raise ValueError("a table named mapped_mirna_* is compared with the known miRNA coordinates and gets four more files: not built")
    words = np.ascontiguousarray(words, dtype=np.uint64)
    if words.ndim != 2:
        raise ValueError("write_predict_features: words must be [W, n]")
    W, n = words.shape
    lens = np.ascontiguousarray(lens, dtype=np.uint8)
    nm = None if nmask is None else np.ascontiguousarray(nmask, dtype=np.uint64)
    counts = np.ascontiguousarray(counts, dtype=np.uint32)
    soff = np.ascontiguousarray(kept_seq_off, dtype=np.uint64)
    orig = np.frombuffer(bytes(kept_orig), dtype=np.uint8)
    cl = {k: np.ascontiguousarray(clusters[k], dtype=dt) for k, dt in
          (("entry", np.uint32), ("strand", np.uint8), ("start", np.uint32), ("end", np.uint32))}
    K = int(soff.shape[0]) - 1
    if lens.shape != (n,) or counts.shape != (n,) or (nm is not None and nm.shape != words.shape):
        raise ValueError("write_predict_features: words [W, n], nmask, lens and counts [n] must match")
    if K < 0 or int(soff[-1]) != orig.shape[0] or (index.n_ref if index is not None else 0) != K or any(a.shape != (K,) for a in cl.values()):
        raise ValueError("write_predict_features: entry, strand, start, end [K], kept_seq_off [K + 1] closing at kept_orig and "
                         "the library's K entries must match")
    G = int(res["n_groups"])
    row_read = np.ascontiguousarray(res["row_read"], dtype=np.uint32)
    row_diag = np.ascontiguousarray(res["row_diag"], dtype=np.int32)
    goff = np.ascontiguousarray(res["group_off"], dtype=np.uint32)
    arr = {k: np.ascontiguousarray(res[k], dtype=dt) for k, dt in
           (("group_cluster", np.uint32), ("frame", np.int32), ("exact", np.uint64), ("nine", np.uint64), ("nb_t", np.uint32),
            ("nb_up", np.int64), ("nb_down", np.int64), ("nb_flags", np.uint8))}
    order = np.ascontiguousarray(res["order"], dtype=np.uint32)
    if row_diag.shape != row_read.shape or (G and goff.shape != (G + 1,)) or arr["frame"].size != 4 * G or arr["nine"].size != 45 * G or \
            any(arr[k].shape[0] != G for k in ("group_cluster", "exact", "nb_t", "nb_up", "nb_down", "nb_flags")):
        raise ValueError("write_predict_features: the row arrays [rows] and the group arrays [G] do not fit each other")
    texts = None
    if group_text:
        texts = (C.c_char_p * max(G, 1))()
        for g, text in group_text.items():
            if not 0 <= int(g) < G:
                raise ValueError("write_predict_features: text for group %d of %d" % (g, G))
            texts[int(g)] = text.encode("ascii")
    hs = (C.c_void_p * max(len(parts), 1))(*[p._h.value for p in parts])
    written = (C.c_uint64 * 2)()
    with _writer_threads(threads):
        rc = lib.mrg_write_predict_features(
            os.fsencode(table_path[:-4] + FEATURES_SUFFIX), os.fsencode(table_path[:-4] + CLUSTER_SUFFIX), int(base[0] == "mapped"), hs,
            len(parts), index._h if index is not None else None, K, _ptr(cl["entry"]), _ptr(cl["strand"]), _ptr(cl["start"]), _ptr(cl["end"]),
            soff.ctypes.data, _ptr(orig), _ptr(words), W, n, _ptr(lens), None if nm is None else _ptr(nm), _ptr(counts), n,
            len(row_read), _ptr(row_read), _ptr(row_diag), G, _ptr(goff), _ptr(arr["group_cluster"]), _ptr(arr["frame"]), _ptr(arr["exact"]),
            _ptr(arr["nine"]), _ptr(arr["nb_t"]), _ptr(arr["nb_up"]), _ptr(arr["nb_down"]), _ptr(arr["nb_flags"]), texts, len(order),
            _ptr(order), written)
    if rc != 0:
        msg = (lib.mrg_last_error() or b"").decode("utf-8", "replace")
        if "leaves its chromosome" in msg:   # (the reference slices a shorter template there and prints garbage)
            raise ValueError(msg)
        _native.check(rc)
    return int(written[0]), int(written[1])


def entry_tables(parts):
    """(entry_len, entry_rank) uint32 over the genome's entries: every entry's length, and the position of its name among
    the names in Python's string order (the order the reference walks the chromosomes in)."""
    from . import _native
    names, lens = [], []
    for ix in parts:
        ln = C.c_uint32()
        for i, nm in enumerate(ix.names):
            _native.check(ix._lib.mrg_index_seq(ix._h, i, None, 0, C.byref(ln)))   # (no buffer: the length alone)
            names.append(nm)
            lens.append(int(ln.value))
    rank = np.zeros(len(names), dtype=np.uint32)
    rank[np.array(sorted(range(len(names)), key=lambda i: names[i]), dtype=np.int64)] = np.arange(len(names), dtype=np.uint32)
    return np.array(lens, dtype=np.uint32), rank


def cluster_features(engine, rs, counts, trim_result, remap_result, parts, out_stem, threads=None, timings=None, keep_device=False):
    """The reference's miRge2.0.py:604 (generate_featureFiles) from the arrays: the rows map_reads_to_clusters left
    (remap_result: its return value with keep_device=True; rs / counts: the reads it mapped) against the clusters the trim
    retained (trim_result: trim_clusters' return value plus "clusters" = retained_clusters(...)) on the genome `parts`.
    Writes `<out_stem>_vs_representative_seq_modified_selected_sorted_features.tsv` and `..._cluster.txt`; returns the dict
    of Engine.predict_features plus seen / passed / written (groups), lines (of `_features.tsv`), host_groups and
    row_status_counts [8].  With no retained cluster or no row the partial header and an empty `_cluster.txt` are written.
    timings gets device_ms, download_ms, host_s and write_s.  keep_device=True adds "device" (Engine.predict_features') and
    "index" (the cluster library) for cluster_precursors; neither is there when nothing was built."""
    import time
    import torch
    table_path = out_stem + REMAP_SUFFIX
    clusters = trim_result.get("clusters")
    K = len(trim_result["kept"])
    if clusters is None or any(len(clusters[k]) != K for k in ("entry", "strand", "start", "end")):
        raise ValueError("cluster_features: the trim result needs \"clusters\" = retained_clusters(...) over its kept clusters")
    n_rows = int(remap_result["n_rows"])
    empty = dict(n_groups=0, n_passed=0, n_sorted=0, seen=0, passed=0, written=0, lines=0, host_groups=0,
                 row_status_counts=np.zeros(8, np.int64))
    if K == 0 or n_rows == 0 or rs is None:
        for suffix, text in ((FEATURES_SUFFIX, _FEATURES_HEADER_HEAD), (CLUSTER_SUFFIX, "")):
            with open(table_path[:-4] + suffix, "w") as fh:
                fh.write(text)
        return empty
    if "device" not in remap_result or "index" not in remap_result:
        raise ValueError("cluster_features: the remap result must come from map_reads_to_clusters(..., keep_device=True)")
    index = remap_result["index"]
    entry_len, entry_rank = entry_tables(parts)
    counts = np.ascontiguousarray(counts.cpu().numpy()).view(np.uint32) if torch.is_tensor(counts) else np.ascontiguousarray(counts, dtype=np.uint32)
    words = rs.words.cpu().numpy().view(np.uint64)
    lens = rs.lens.cpu().numpy()
    nmask = None if rs.nmask is None else rs.nmask.cpu().numpy().view(np.uint64)
    row_read = remap_result["rows"][0]
    soff = np.ascontiguousarray(trim_result["kept_seq_off"], dtype=np.uint64)
    orig = bytes(trim_result["kept_orig"])
    texts, host_s = {}, [0.0]

    def host_groups(g, lo, hi, c):
        t0 = time.perf_counter()
        members = [int(r) for r in row_read[lo:hi]]
        seqs = pack.unpack_reads(words[:, members], lens[members], None if nmask is None else nmask[:, members])
        rows, numbers = host_group(orig[int(soff[c]):int(soff[c + 1])].decode("ascii"), seqs, counts[members])
        texts[g] = "\n".join(rows)
        host_s[0] += time.perf_counter() - t0
        return numbers
    cl = dict(clusters, kept=trim_result["kept"], kept_seq_off=soff, kept_orig=orig)
    res = engine.predict_features(rs, counts, remap_result["device"][:2], cl, entry_len, entry_rank, host_groups, timings,
                                  **({"keep_device": True} if keep_device else {}))
    res["row_read"] = row_read
    if keep_device:
        res["index"] = index
    t0 = time.perf_counter()
    blocks, lines = write_predict_features(table_path, parts, index, clusters, soff, orig, words, lens, nmask, counts, res, texts, threads)
    if timings is not None:
        timings.update(host_s=host_s[0], write_s=time.perf_counter() - t0)
    res.update(seen=res["n_groups"], passed=res["n_passed"], written=blocks, lines=lines, host_groups=len(texts),
               row_status_counts=np.bincount(res["row_status"], minlength=8))
    return res


PRECURSOR_SUFFIX = "_features_precusor.fa"


def write_precursors(path, parts, index, cl_entry, group_cluster, rec, threads=None):
    """mrg_write_precursors: the file `path` from host arrays -- the genome's parts, the cluster library (entry j's name is
    retained cluster j's), every retained cluster's entry, every group's cluster and rec = a dict of rec_group, rec_lo,
    rec_hi [2 W], rec_off [2 W + 1] and seq (bytes) as Engine.predict_precursors returns them.  Returns (records, bytes)."""
    from . import _native
    lib = _native.load()
    cl_entry = np.ascontiguousarray(cl_entry, dtype=np.uint32)
    group_cluster = np.ascontiguousarray(group_cluster, dtype=np.uint32)
    rg, lo, hi = (np.ascontiguousarray(rec[k], dtype=np.uint32) for k in ("rec_group", "rec_lo", "rec_hi"))
    off = np.ascontiguousarray(rec["rec_off"], dtype=np.uint64)
    seq = np.frombuffer(bytes(rec["seq"]), dtype=np.uint8)
    n_rec = int(rg.shape[0])
    if lo.shape != (n_rec,) or hi.shape != (n_rec,) or off.shape != (n_rec + 1,):
        raise ValueError("write_precursors: rec_group, rec_lo, rec_hi [records] and rec_off [records + 1] must match")
    if int(off[-1]) != seq.shape[0]:
        raise ValueError("write_precursors: rec_off must close at the %d sequence bytes (it ends at %d)" % (seq.shape[0], int(off[-1])))
    K = int(cl_entry.shape[0])
    if (index.n_ref if index is not None else 0) != K:
        raise ValueError("write_precursors: the cluster library's entries must be the %d retained clusters" % K)
    hs = (C.c_void_p * max(len(parts), 1))(*[p._h.value for p in parts])
    written = (C.c_uint64 * 2)()
    with _writer_threads(threads):
        _native.check(lib.mrg_write_precursors(
            os.fsencode(path), hs, len(parts), index._h if index is not None else None, K, _ptr(cl_entry), int(group_cluster.shape[0]),
            _ptr(group_cluster), n_rec, _ptr(rg), _ptr(lo), _ptr(hi), off.ctypes.data, _ptr(seq), int(seq.shape[0]), written))
    return int(written[0]), int(written[1])


def cluster_precursors(engine, features_result, trim_result, parts, out_stem, threads=None, timings=None, parts_libs=None):
    """The reference's miRge2.0.py:608 (get_precursors) from the arrays: for every line cluster_features wrote, the two
    genome windows around the stable part of the cluster, as RNA -- the file RNAfold is fed.  features_result: what
    cluster_features(..., keep_device=True) returned (its "device" and "index"); trim_result: as cluster_features takes it;
    parts: the genome's FmIndex list, resident on `engine` (parts_libs: their keys there; None: looked up by object).
    Writes `<out_stem>_vs_representative_seq_modified_selected_sorted_features_precusor.fa`; returns the dict of
    Engine.predict_precursors plus records and bytes (of the file).  timings gets device_ms, download_ms and write_s."""
    import time
    path = out_stem + REMAP_SUFFIX[:-4] + PRECURSOR_SUFFIX
    dev = features_result.get("device")
    if dev is None:   # (no retained cluster or no row: the feature file is its header)
        with open(path, "w"):
            pass
        return dict(written=np.zeros(0, np.uint8), rec_group=np.zeros(0, np.uint32), rec_lo=np.zeros(0, np.uint32),
                    rec_hi=np.zeros(0, np.uint32), rec_off=np.zeros(1, np.uint64), seq=b"", n_written=0, device_ms=None,
                    download_ms=None, records=0, bytes=0)
    if parts_libs is None:
        by_id = {id(ix): k for k, ix in engine.indexes.items()}
        try:
            parts_libs = [by_id[id(ix)] for ix in parts]
        except KeyError:
            raise ValueError("cluster_precursors: a genome part is not resident on this engine (genome_libraries adds them)")
    res = engine.predict_precursors(dev, None, None, parts_libs, timings)
    if int(res["written"].sum()) != int(features_result["lines"]):
        raise ValueError("cluster_precursors: %d groups written, the feature file holds %d lines" % (int(res["written"].sum()),
                                                                                                  int(features_result["lines"])))
    t0 = time.perf_counter()
    records, nbytes = write_precursors(path, parts, features_result["index"], trim_result["clusters"]["entry"],
                                       features_result["group_cluster"], res, threads)
    if timings is not None:
        timings["write_s"] = time.perf_counter() - t0
    res.update(records=records, bytes=nbytes)
    return res


def rename_str_file(fasta, str_tmp, str_out):
    """The reference's renameStrFile (miRge2.0.py:612) for users who fold `_precusor.fa` with their own RNAfold: RNAfold
    cuts the names short, so every three-line record of `str_tmp` (name, sequence, structure) gets the name line of the
    record at the same position of `fasta` back.  Pure host code; writes `str_out`, returns the records written."""
    with open(fasta) as fh:
        names = fh.readlines()[0::2]
    with open(str_tmp) as fh:
        lines = fh.readlines()
    n = (len(lines) + 2) // 3
    if n > len(names):
        raise ValueError("rename_str_file: %d folded records for %d sequences" % (n, len(names)))
    with open(str_out, "w") as out:
        for i in range(n):
            out.write(names[i])
            out.writelines(lines[3 * i + 1:3 * i + 3])
    return n


def screen_precursors(engine, features_result, precursors_result, fold, out_stem, pruned_length=15, threads=None, timings=None):
    """The reference's miRge2.0.py:610-626 (RNAfold, renameStrFile, screen_precusor_candidates) from the arrays, with two
    fold calls a sample.  features_result / precursors_result: what cluster_features (nb_flags, nb_up, nb_down) and
    cluster_precursors (rec_group, records) returned; fold: a callable (fasta_path, str_path), or RNAfold's path.
    Writes `_features_precusor_tmp.str`, `_features_precusor.str`, `_features_pruned_<length>.fa` / `.str` and
    `<table>_features_updated_stableClusterSeq_<length>.tsv`; candidates beyond the kernels' limits go through host_prune /
    host_screen_features.  Returns a dict: lines, candidates, pruned (folded again), host_candidates, folds, best, path.
    timings gets fold1_s, fold2_s, parse_s, device_s (the device calls with their transfers), host_s and write_s."""
    import time
    if isinstance(fold, (str, bytes, os.PathLike)):
        fold = fold_command(os.fspath(fold))
    stem = out_stem + REMAP_SUFFIX[:-4]
    features_path, fasta = stem + FEATURES_SUFFIX, stem + PRECURSOR_SUFFIX
    out_path = stem + "_features_updated_stableClusterSeq_%d.tsv" % int(pruned_length)
    t = dict(fold1_s=0.0, fold2_s=0.0, parse_s=0.0, device_s=0.0, host_s=0.0, write_s=0.0)
    clock = time.perf_counter
    n_rec = int(precursors_result["records"])
    n = n_rec // 2
    if n == 0:   # (the feature file is its header: nothing to fold)
        write_screened_features(features_path, out_path, np.zeros(0, np.int32), np.zeros((0, 16), np.int32), np.zeros(1, np.uint64), b"", b"",
                                np.zeros(0), threads)
        if timings is not None:
            timings.update(t)
        return dict(lines=0, candidates=0, pruned=0, host_candidates=0, folds=0, best=np.zeros(0, np.int32), path=out_path)
    t0 = clock()
    fold(fasta, stem + "_features_precusor_tmp.str")
    t["fold1_s"] = clock() - t0
    t0 = clock()
    rename_str_file(fasta, stem + "_features_precusor_tmp.str", stem + "_features_precusor.str")
    rec_off, rec_seq, rec_str, rec_mfe = read_str_file(stem + "_features_precusor.str", n_rec)
    with open(features_path) as fh:
        rows = fh.read().split("\n")
    col = rows[0].strip().split("\t").index("stableClusterSeq")
    mirnas = [r.strip().split("\t")[col].replace("T", "U").encode("ascii") for r in rows[1:] if r != ""]
    if len(mirnas) != n:
        raise ValueError("screen_precursors: %d feature lines, %d precursor records" % (len(mirnas), n_rec))
    mir_off = np.zeros(n + 1, np.uint64)
    mir_off[1:] = np.cumsum([len(m) for m in mirnas])
    mir = b"".join(mirnas)
    t["parse_s"] = clock() - t0
    t0 = clock()
    line_group = np.ascontiguousarray(precursors_result["rec_group"][0::2], dtype=np.uint32)
    cands = engine.predict_screen_candidates(line_group, features_result["nb_flags"], features_result["nb_up"], features_result["nb_down"])
    pr = engine.predict_screen_prune(cands["cand_rec"], cands["cand_mir"], rec_off, rec_seq, rec_str, mir_off, mir, pruned_length)
    cand_rec = cands["cand_rec"].cpu().numpy().view(np.uint32)
    cand_mir = cands["cand_mir"].cpu().numpy().view(np.uint32).reshape(-1, 2)
    t["device_s"] += clock() - t0
    status, p_off, p_seq = pr["status"].copy(), pr["pruned_off"], pr["pruned"]
    text = lambda blob, off, k: blob[int(off[k]):int(off[k + 1])].decode("ascii")
    mirnas_of = lambda c: [text(mir, mir_off, int(m)) for m in cand_mir[c] if m != 0xffffffff]
    todo = np.flatnonzero(status == 2)
    host_candidates = set(int(c) for c in todo)
    if todo.size:   # the pruned bytes again, with the host's slices in their places
        t0 = clock()
        parts = [p_seq[int(p_off[c]):int(p_off[c + 1])] for c in range(4 * n)]
        for c in todo:
            r = int(cand_rec[c])
            cut = host_prune(text(rec_seq, rec_off, r), text(rec_str, rec_off, r), mirnas_of(c), pruned_length)
            status[c] = 0 if cut is None else 1
            if cut is not None:
                parts[c] = rec_seq[int(rec_off[r]) + cut[0]:int(rec_off[r]) + cut[1]]
        p_off = np.zeros(4 * n + 1, np.uint64)
        p_off[1:] = np.cumsum([len(p) for p in parts])
        p_seq = b"".join(parts)
        t["host_s"] += clock() - t0
    keep = (status == 1) & (np.diff(p_off.astype(np.int64)) > 0)   # (an empty slice folds to nothing: the all-None row)
    pruned_fa = stem + "_features_pruned_%d.fa" % int(pruned_length)
    n_pruned = write_pruned_fasta(pruned_fa, p_off, p_seq, keep)
    t0 = clock()
    fold(pruned_fa, pruned_fa[:-3] + ".str")
    t["fold2_s"] = clock() - t0
    t0 = clock()
    f_off, f_seq, p_str, f_mfe = read_str_file(pruned_fa[:-3] + ".str", n_pruned)
    if f_seq != p_seq:
        raise ValueError("screen_precursors: %s does not hold the sequences of %s" % (pruned_fa[:-3] + ".str", pruned_fa))
    p_mfe = np.zeros(4 * n, np.float64)
    p_mfe[keep] = f_mfe
    t["parse_s"] += clock() - t0
    t0 = clock()
    feat = engine.predict_screen_features(keep.astype(np.uint8), cands["cand_mir"], p_off, p_seq, p_str, mir_off, mir)
    t["device_s"] += clock() - t0
    t0 = clock()
    for c in np.flatnonzero(feat[:, 0] == 2):
        host_candidates.add(int(c))
        row = host_screen_features(text(p_seq, p_off, c), text(p_str, p_off, c), mirnas_of(c))
        feat[c] = 0 if row is None else row
    t["host_s"] += clock() - t0
    t0 = clock()
    best = engine.predict_screen_select(cands["cand_n"], cands["cand_rec"], rec_mfe, feat, 19 - 1 - 3)
    t["device_s"] += clock() - t0
    t0 = clock()
    lines = write_screened_features(features_path, out_path, best, feat, p_off, p_seq, p_str, p_mfe, threads)
    t["write_s"] = clock() - t0
    if timings is not None:
        timings.update(t, host_candidates=len(host_candidates))
    return dict(lines=lines, candidates=int((status != 3).sum()), pruned=n_pruned, host_candidates=len(host_candidates), folds=2, best=best,
                path=out_path)


def fold_command(cmd):
    """The default `fold` of screen_precursors: a callable (fasta_path, str_path) that starts `cmd --noPS --noLP` once,
    without a shell, the FASTA on its standard input and the answer written to str_path."""
    import subprocess

    def fold(fasta_path, str_path):
        with open(fasta_path, "rb") as src, open(str_path, "wb") as dst:
            done = subprocess.run([cmd, "--noPS", "--noLP"], stdin=src, stdout=dst)
        if done.returncode != 0:
            raise OSError("%s --noPS --noLP left with status %d" % (cmd, done.returncode))
    return fold


def resolve_fold_cmd(rnafold_dir=None, fold_cmd=None):
    """The executable --novel-screen folds with: fold_cmd, else <rnafold_dir>/RNAfold (the reference's -pr).  ValueError
    with the reference's message when neither names an executable file."""
    cmd = fold_cmd if fold_cmd else (os.path.join(rnafold_dir, "RNAfold") if rnafold_dir else None)
    if cmd and os.path.isfile(cmd) and os.access(cmd, os.X_OK):
        return os.path.abspath(cmd)
    raise ValueError("RNAfold can't be found in %s. Please check it." % (os.path.dirname(cmd) if fold_cmd else rnafold_dir))


def read_str_file(path, expected):
    """mrg_read_str_file: the records of an RNAfold output as arrays -- (off uint64 [n + 1], seq bytes, structure bytes, mfe
    float64 [n]).  MirgeAmdError naming both counts when the file does not hold `expected` records."""
    from . import _native
    lib = _native.load()
    n, length, h = C.c_uint64(), C.c_uint64(), C.c_void_p()
    _native.check(lib.mrg_read_str_file(os.fsencode(path), int(expected), C.byref(n), C.byref(length), C.byref(h)))
    try:
        off, mfe = np.zeros(n.value + 1, np.uint64), np.zeros(n.value, np.float64)
        seq, structure = np.zeros(max(length.value, 1), np.uint8), np.zeros(max(length.value, 1), np.uint8)
        _native.check(lib.mrg_str_file_copy(h, off.ctypes.data, seq.ctypes.data, structure.ctypes.data, mfe.ctypes.data))
    finally:
        lib.mrg_str_file_free(h)
    return off, seq[:length.value].tobytes(), structure[:length.value].tobytes(), mfe


def write_pruned_fasta(path, off, seq, keep):
    """mrg_write_pruned_fasta: `>c<k>` and string k (bytes [off[k], off[k + 1]) of seq) for every k with keep[k]."""
    from . import _native
    lib = _native.load()
    off = np.ascontiguousarray(off, dtype=np.uint64)
    keep = np.ascontiguousarray(keep, dtype=np.uint8)
    buf = np.frombuffer(bytes(seq), dtype=np.uint8)
    if off.shape[0] != keep.shape[0] + 1 or int(off[-1]) != buf.shape[0]:
        raise ValueError("write_pruned_fasta: off [n + 1] must close at the sequence bytes and keep hold n flags")
    written = C.c_uint64()
    _native.check(lib.mrg_write_pruned_fasta(os.fsencode(path), int(keep.shape[0]), off.ctypes.data, _ptr(buf), _ptr(keep), C.byref(written)))
    return int(written.value)


def write_screened_features(features_path, out_path, best, feat, p_off, p_seq, p_str, p_mfe, threads=None):
    """mrg_write_screened_features: the feature file's lines, each with the 14 columns of its chosen candidate.  best [n],
    feat [4 n, 16], p_off [4 n + 1] into p_seq / p_str, p_mfe [4 n].  Returns the lines written."""
    from . import _native
    lib = _native.load()
    best = np.ascontiguousarray(best, dtype=np.int32)
    feat = np.ascontiguousarray(feat, dtype=np.int32).reshape(-1)
    p_off = np.ascontiguousarray(p_off, dtype=np.uint64)
    p_mfe = np.ascontiguousarray(p_mfe, dtype=np.float64)
    seq, structure = (np.frombuffer(bytes(b), dtype=np.uint8) for b in (p_seq, p_str))
    n = int(best.shape[0])
    if feat.shape[0] != 64 * n or p_off.shape[0] != 4 * n + 1 or p_mfe.shape[0] != 4 * n or int(p_off[-1]) != seq.shape[0] or \
            seq.shape != structure.shape:
        raise ValueError("write_screened_features: best [n], feat [4 n, 16], p_off [4 n + 1] closing at p_seq and p_str, p_mfe [4 n] must match")
    written = C.c_uint64()
    with _writer_threads(threads):
        _native.check(lib.mrg_write_screened_features(os.fsencode(features_path), os.fsencode(out_path), n, _ptr(best), _ptr(feat),
                                                      p_off.ctypes.data, _ptr(seq), _ptr(structure), _ptr(p_mfe), C.byref(written)))
    return int(written.value)


def classifier_files(model_dir, species):
    """The model file of `species` and the namelist from `model_dir`, opened and validated: (svm_model.SvmModel, names).
    No GPU is touched: the callers run this before any device work, as they check RNAfold.  OSError or ValueError."""
    from . import svm_model
    if not model_dir:
        raise ValueError("the classification needs the directory of the model files (miRge2.0's models/)")
    return svm_model.load_model(model_dir, species), svm_model.read_namelist(model_dir)


def classified_paths(screened_path):
    """The five files preprocess_featureFiles and model_predict write next to the screened table, by the reference's names."""
    d, base = os.path.dirname(screened_path), os.path.basename(screened_path)
    tmp = "_".join(base.split("_")[:-9]) + "_dataset_" + base.split("_")[-1].split(".")[0]
    sample = "_".join((tmp + "_refined_features.csv").split("_")[2:-5])
    return dict(dataset=os.path.join(d, tmp + ".csv"), refined_tmp=os.path.join(d, tmp + "_refined_tmp.csv"),
                refined=os.path.join(d, tmp + "_refined_features.csv"), detailed=os.path.join(d, "predicted_" + sample + "_detailed.csv"),
                novel=os.path.join(d, sample + "_novel_miRNAs_miRge2.0.csv"))


class ScreenedTable:
    """mrg_predict_model_filter: a screened table read by the native reader, which writes the reference's three filter files
    (paths["dataset"], ["refined_tmp"], ["refined"]) on the way.  rows: the table's, the first filter's and the second's row
    counts; stray: the selected names whose column holds a cell that is no number (0 for every row); x: the raw feature rows
    [refined, nf] for the model's selected names.  write() is mrg_predict_model_write.  A context manager: the native side is
    released on exit."""

    def __init__(self, screened_path, model, namelist):
        from . import _native
        self._lib = _native.load()
        self.paths = classified_paths(screened_path)
        counts, self._h = (C.c_uint64 * 4)(), C.c_void_p()
        enc = lambda names: "\n".join(names).encode("utf-8")
        nf = len(model.feature_names)
        _native.check(self._lib.mrg_predict_model_filter(
            os.fsencode(screened_path), os.fsencode(self.paths["dataset"]), os.fsencode(self.paths["refined_tmp"]),
            os.fsencode(self.paths["refined"]), enc(namelist), enc(model.feature_names), nf, counts, C.byref(self._h)))
        self.rows, self.stray = tuple(int(c) for c in counts[:3]), int(counts[3])
        self.x = np.zeros((self.rows[2], nf), np.float64)
        try:
            _native.check(self._lib.mrg_predict_model_rows(self._h, _ptr(self.x.reshape(-1))))
        except Exception:
            self.close()
            raise

    def write(self, pred, prob, threads=None):
        """`predicted_<sample>_detailed.csv` and `<sample>_novel_miRNAs_miRge2.0.csv` from pred [n] (1 or -1) and prob [n, 2]
        (class -1, class 1).  Returns (rows predicted 1, rows of the novel list)."""
        from . import _native
        pred = np.ascontiguousarray(pred, dtype=np.int8)
        prob = np.ascontiguousarray(prob, dtype=np.float64).reshape(-1)
        if pred.shape != (self.rows[2],) or prob.shape != (2 * self.rows[2],):
            raise ValueError("ScreenedTable.write: pred [n] and prob [n, 2] for the table's %d refined rows" % self.rows[2])
        predicted, kept = C.c_uint64(), C.c_uint64()
        with _writer_threads(threads):
            _native.check(self._lib.mrg_predict_model_write(self._h, _ptr(pred), _ptr(prob), os.fsencode(self.paths["detailed"]),
                                                            os.fsencode(self.paths["novel"]), C.byref(predicted), C.byref(kept)))
        return int(predicted.value), int(kept.value)

    def close(self):
        if self._h:
            self._lib.mrg_predict_model_free(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def classify_candidates(engine, screened_path, model_dir, species, threads=None, timings=None, classifier=None):
    """The reference's miRge2.0.py:647-648 (preprocess_featureFiles, model_predict) for one screened table
    `*_features_updated_stableClusterSeq_15.tsv`: the three filter files by the native reader (ScreenedTable), the SVM on the
    device (Engine.predict_svm) and `predicted_<sample>_detailed.csv` / `<sample>_novel_miRNAs_miRge2.0.csv` by the native
    writer.  classifier: what classifier_files returned (None: read from model_dir now).  Returns a dict: table, dataset,
    refined (rows per filter), stray (selected names whose column holds a cell that is no number: 0 for every row),
    predicted (rows predicted 1), kept (rows of the novel list), paths, screened (the table's own path), and the device's pred, dec
    and prob.  timings gets
    read_s, device_s and write_s."""
    import time
    model, namelist = classifier if classifier is not None else classifier_files(model_dir, species)
    clock = time.perf_counter
    t0 = clock()
    with ScreenedTable(screened_path, model, namelist) as table:
        t1 = clock()
        res = engine.predict_svm(table.x, model)
        t2 = clock()
        predicted, kept = table.write(res["pred"], res["prob"], threads)
        t3 = clock()
        if timings is not None:
            timings.update(read_s=t1 - t0, device_s=t2 - t1, write_s=t3 - t2)
        return dict(table=table.rows[0], dataset=table.rows[1], refined=table.rows[2], stray=table.stray, predicted=predicted, kept=kept,
                    paths=table.paths, screened=screened_path, pred=res["pred"], dec=res["dec"], prob=res["prob"])


# ------------------------------------------------------------------------------------------------ the report
REPORT_ARRAYS = ("flags", "rank", "up", "down", "pos", "adj", "reads", "gid3", "t_off", "text", "blk", "r_off", "row_start", "row_end",
                 "row_count", "row_soff", "row_text")   # include/mirge_amd.h: MRG_REPORT_*
_REPORT_DTYPES = dict(flags=np.uint8, rank=np.uint32, up=np.int64, down=np.int64, pos=np.int64, adj=np.int32, reads=np.int64, gid3=np.uint32,
                      t_off=np.uint64, text=np.uint8, blk=np.uint8, r_off=np.uint64, row_start=np.int64, row_end=np.int64, row_count=np.int64,
                      row_soff=np.uint64, row_text=np.uint8)


def report_paths(novel_path, table_path, cluster_path):
    """The three files of the report by the reference's names: the table's `_corrected.tsv`; `<sample>_novel_miRNAs_report.csv` and
    the extension `<sample>_novel_miRNAs_report_profiles.tsv` next to the cluster file, under the novel list's stem."""
    stem = os.path.join(os.path.split(os.path.abspath(cluster_path))[0], "_".join(novel_path.split("_")[:-3]))
    return dict(corrected=table_path[:-4] + "_corrected.tsv", report=stem + "_novel_miRNAs_report.csv",
                profiles=stem + "_novel_miRNAs_report_profiles.tsv")


def _report_cluster_path(table_path):
    """`*_cluster.txt` next to a screened table `*_features_updated_stableClusterSeq_<n>.tsv`, by the reference's names."""
    at = table_path.rfind("_features_updated_stableClusterSeq_")
    if at < 0:
        raise ValueError("report_candidates: %s is not a *_features_updated_stableClusterSeq_<n>.tsv; name the cluster file" % table_path)
    return table_path[:at] + "_cluster.txt"


class ReportInputs:
    """mrg_predict_report_read: the novel list, the screened table and the cluster file read, validated and interned by the native
    reader.  n, n_listed, n_rows; arrays: the reader's arrays as numpy copies (REPORT_ARRAYS).  write() is
    mrg_predict_report_write.  A context manager: the native side is released on exit.  ValueError for files the reader refuses."""

    def __init__(self, novel_path, table_path, cluster_path):
        from . import _native
        self._lib = _native.load()
        self.paths = report_paths(novel_path, table_path, cluster_path)
        counts, self._h = (C.c_uint64 * 3)(), C.c_void_p()
        rc = self._lib.mrg_predict_report_read(os.fsencode(novel_path), os.fsencode(table_path), os.fsencode(cluster_path), counts,
                                               C.byref(self._h))
        if rc == _native.MRG_ERR_ARG:
            raise ValueError(self._lib.mrg_last_error().decode("utf-8", "replace"))
        _native.check(rc)
        self.n, self.n_listed, self.n_rows = (int(c) for c in counts)
        self.arrays = {}
        for which, key in enumerate(REPORT_ARRAYS):
            data, size = C.c_void_p(), C.c_uint64()
            _native.check(self._lib.mrg_predict_report_array(self._h, which, C.byref(data), C.byref(size)))
            raw = C.string_at(data, size.value) if size.value else b""
            self.arrays[key] = np.frombuffer(raw, dtype=_REPORT_DTYPES[key]).copy()

    def strings(self, j):
        """(precursor, structure, clusterSeq, stableClusterSeq) of line j."""
        o, text = self.arrays["t_off"], self.arrays["text"]
        return tuple(text[int(o[4 * j + k]):int(o[4 * j + k + 1])].tobytes().decode("ascii", "replace") for k in range(4))

    def rows(self, j):
        """(RNA, start, end, count) of every read row of line j's block."""
        a = self.arrays
        return [(a["row_text"][int(a["row_soff"][r]):int(a["row_soff"][r + 1])].tobytes().decode("ascii", "replace"), int(a["row_start"][r]),
                 int(a["row_end"][r]), int(a["row_count"][r])) for r in range(int(a["r_off"][j]), int(a["r_off"][j + 1]))]

    def write(self, res, threads=None):
        """The three files from Engine.predict_report's arrays."""
        from . import _native
        E = int(res["n_entries"])
        c = lambda key, dt: np.ascontiguousarray(res[key], dtype=dt).reshape(-1)
        src, state, pos_adj = c("src", np.uint32), c("state", np.uint8), c("pos_adj", np.int64)
        if src.shape != (self.n,) or state.shape != (self.n,) or pos_adj.shape != (2 * self.n,):
            raise ValueError("ReportInputs.write: src, state [n] and pos_adj [n, 2] for the table's %d lines" % self.n)
        ent_m, ent_p, row_off, prof_off = c("ent_m", np.uint32), c("ent_p", np.int32), c("row_off", np.uint64), c("prof_off", np.uint64)
        lead, trail, prof, total, flag = c("lead", np.int32), c("trail", np.int32), c("prof", np.uint64), c("total", np.uint64), c("flag", np.uint8)
        if ent_m.shape != (E,) or ent_p.shape != (E,) or row_off.shape != (E + 1,) or prof_off.shape != (E + 1,) or total.shape != (E,) or \
                flag.shape != (E,) or lead.shape != (int(row_off[E]),) or trail.shape != lead.shape or prof.shape != (int(prof_off[E]),):
            raise ValueError("ReportInputs.write: the entries' arrays do not match each other")
        with _writer_threads(threads):
            rc = self._lib.mrg_predict_report_write(self._h, _ptr(src), _ptr(state), _ptr(pos_adj), E, _ptr(ent_m), _ptr(ent_p), _ptr(row_off),
                                                    _ptr(lead), _ptr(trail), _ptr(prof_off), _ptr(prof), _ptr(total), _ptr(flag),
                                                    os.fsencode(self.paths["corrected"]), os.fsencode(self.paths["report"]),
                                                    os.fsencode(self.paths["profiles"]))
        if rc == _native.MRG_ERR_ARG:
            raise ValueError(self._lib.mrg_last_error().decode("utf-8", "replace"))
        _native.check(rc)

    def close(self):
        if self._h:
            self._lib.mrg_predict_report_free(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def host_report_line(seq, structure, cluster_seq, stable):
    """The arm re-type and the stable index of one line, for lines beyond the kernel's limits: (True when the stretch of the
    structure under clusterSeq (T as U) holds a `(` before a `)`, where the precursor holds stableClusterSeq (T as U) or -1)."""
    rna = cluster_seq.replace("T", "U")
    start = seq.find(rna)
    stretch = structure[start:start + len(rna)]
    first = stretch.find("(")
    return first >= 0 and stretch.rfind(")") > first, seq.find(stable.replace("T", "U"))


def host_report_entry(precursor, clusters):
    """The padded rows and the profile of one entry, for entries beyond the kernel's limits.  clusters: per cluster (the mature's,
    then the passenger's) (rows, stable index, stable length, start, end, minus).  Returns (lead, trail, sums, total, ragged)."""
    L = len(precursor)
    lead, trail, sums, total, ragged = [], [], [0] * L, 0, False
    for rows, at, stable_len, start, end, minus in clusters:
        head, tail = at, L - at - stable_len
        p_head, p_tail = (start - tail, end + head) if minus else (start - head, end + tail)
        for seq, r_start, r_end, count in rows:
            before, behind = max(0, r_start - p_head), max(0, p_tail - r_end)
            ld, tr = (behind, before) if minus else (before, behind)
            lead.append(ld)
            trail.append(tr)
            total += count
            ragged = ragged or ld + len(seq) + tr != L
            for q in range(min(L, ld + len(seq) + tr)):
                ch = seq[q - ld] if ld <= q < ld + len(seq) else "-"
                if ch == precursor[q]:
                    sums[q] += count
    return lead, trail, sums, total, ragged


def report_candidates(engine, source, threads=None, timings=None):
    """The reference's miRge2.0.py:652 (write_novel_report) without its drawing.  source: classify_candidates' result, or a dict
    with the paths `novel` (`<sample>_novel_miRNAs_miRge2.0.csv`), `table` (`*_features_updated_stableClusterSeq_15.tsv`) and
    `cluster` (`*_modified_selected_sorted_cluster.txt`; default: next to the table under the reference's name).  The native
    reader (ReportInputs), the pair correction, the arm re-type, the entries and the coverage profiles on the device
    (Engine.predict_report) and the native writers: the table's `_corrected.tsv` and `<sample>_novel_miRNAs_report.csv`, byte for
    byte the reference's, and the extension `<sample>_novel_miRNAs_report_profiles.tsv` (what the PDFs plot).  The PDFs are not
    drawn.  Returns a dict: entries, lines, listed, host_lines and host_entries (worked out by the Python restatement: a precursor
    beyond 256 characters, a clusterSeq or read beyond 255), paths, and the device's arrays.  timings gets read_s, device_s and
    write_s.  ValueError, naming the line and the reason, where the reference raises; no file is written then."""
    import time
    paths = source.get("paths", source)
    novel, table = paths["novel"], paths.get("table", source.get("screened"))
    if table is None:
        raise ValueError("report_candidates: the path of the screened table is missing")
    cluster = paths.get("cluster") or _report_cluster_path(table)
    clock = time.perf_counter
    t0 = clock()
    with ReportInputs(novel, table, cluster) as inputs:
        a = inputs.arrays
        t1 = clock()

        def host_line(j, src):
            seq, structure = inputs.strings(src)[:2]
            _, _, cluster_seq, stable = inputs.strings(j)
            return host_report_line(seq, structure, cluster_seq, stable)

        def host_entry(e, m, p, src, pos_adj, stable_idx):
            clusters = [(inputs.rows(x), int(stable_idx[x]), len(inputs.strings(x)[3]), int(pos_adj[x][0]), int(pos_adj[x][1]),
                         bool(a["flags"][x] & 32)) for x in ((m,) if p < 0 else (m, p))]
            return host_report_entry(inputs.strings(int(src[m]))[0], clusters)
        res = engine.predict_report(a, host_line=host_line, host_entry=host_entry)
        t2 = clock()
        inputs.write(res, threads)
        t3 = clock()
        if timings is not None:
            timings.update(read_s=t1 - t0, device_s=t2 - t1, write_s=t3 - t2)
        return dict(res, entries=res["n_entries"], lines=inputs.n, listed=inputs.n_listed, paths=dict(inputs.paths, novel=novel, table=table,
                                                                                                         cluster=cluster))


def _partners(structure):
    """{position: partner} of a dot-bracket structure; ValueError where the brackets do not balance."""
    open_at, pairs = [], {}
    for x, ch in enumerate(structure):
        if ch == "(":
            open_at.append(x)
        elif ch == ")":
            if not open_at:
                raise ValueError("the structure's brackets do not balance")
            y = open_at.pop()
            pairs[x], pairs[y] = y, x
    if open_at:
        raise ValueError("the structure's brackets do not balance")
    return pairs


def _arm(stretch):
    """checkArm over the miRNA's stretch of the structure: 0 loop, 1 arm5, 2 arm3, 3 unmatchedRegion."""
    first, last = stretch.find("("), stretch.rfind(")")
    if first >= 0 and last > first:
        return 0
    if first >= 0:
        return 1 if stretch.count("(") >= stretch.count(")") else 2
    return 2 if last >= 0 else 3


def host_prune(seq, structure, mirnas, pruned_length=15):
    """The host's getPrunedPrecusor up to the fold, for the candidates the kernels leave (beyond 256 characters): the slice
    (lo, hi) of the record with 0 <= lo <= hi <= len, or None where pairing_partner gives None."""
    chosen = mirnas[0] if len(mirnas) == 1 or seq.find(mirnas[0]) == 20 else mirnas[1]
    start = seq.find(chosen)
    end = start + len(chosen)
    pairs = _partners(structure)
    if _arm(structure[start:end]) == 1:
        at = structure.index("(", start, end)
        cut = slice(start - pruned_length, min(at - start + pairs[at], len(seq) - 1) + 1 + pruned_length)
    else:
        if end - 1 >= len(structure):
            raise ValueError("an absent miRNA longer than the sequence: the reference dies of an IndexError")
        at = structure.rfind(")", 0, max(end, 0))
        if at < 0:
            return None
        cut = slice(max(pairs[at] - (end - 1 - at), 0) - pruned_length, end + pruned_length)
    lo, hi, _ = cut.indices(len(seq))
    return lo, max(lo, hi)


def host_screen_features(seq, structure, mirnas):
    """The host's featuresInPrecusor / percentageOfPairedInMiRNA / bindingsInMiRNA for the candidates the kernels leave:
    the 16 words of a feature row (state 1), or None for the all-None row.  Every position gets its element's letter and
    the LAST character of the element's number, as the reference's to_element_string does: from ten stems (or hairpins) on
    two elements share a key, their adjacent runs merge and stemLen takes one maximum for both."""
    if "(" not in structure or ")" not in structure:
        return None
    pairs = _partners(structure)
    n = len(structure)
    label = [""] * n
    n_hairpin = n_stem = interior = 0
    for x in range(n):
        if structure[x] != "(":
            continue
        y = pairs[x]
        nxt = x + 1
        while structure[nxt] == ".":
            nxt += 1
        if nxt == y:
            if y - x - 1 < 3:
                raise ValueError("a hairpin loop under 3")
            for z in range(x + 1, y):
                label[z] = "h" + str(n_hairpin)[-1]
            n_hairpin += 1
        else:
            back = pairs[nxt] + 1
            while structure[back] == ".":
                back += 1
            if back == y and (nxt > x + 1 or pairs[nxt] < y - 1):
                interior += 1
        if not (x and structure[x - 1] == "(" and pairs[x - 1] == y + 1):
            z = 0
            while structure[x + z] == "(" and pairs[x + z] == y - z:
                label[x + z] = label[y - z] = "s" + str(n_stem)[-1]
                z += 1
            n_stem += 1
    runs, order = {}, []
    for x in range(n):
        if label[x] and (x == 0 or label[x - 1] != label[x]):
            if label[x] not in runs:
                runs[label[x]] = []
                order.append(label[x])
            runs[label[x]].append([x, x])
        elif label[x]:
            runs[label[x]][-1][1] = x
    loops = [r for key in order if key[0] == "h" for r in runs[key]]
    row = [0] * 16
    row[0], row[1], row[2], row[3] = 1, n_hairpin, max(structure.count("("), structure.count(")")), interior
    row[5] = max(r[1] - r[0] + 1 for r in loops)
    row[8] = -1
    for t, mirna in enumerate(mirnas):
        start = seq.find(mirna)
        last = start + len(mirna) - 1
        arm = _arm(structure[start:start + len(mirna)])
        shared = [max(0, min(last, r[1]) - max(start, r[0]) + 1) for r in loops]
        gap = [r[0] - 1 - last if arm == 1 else start - r[1] - 1 for r in loops]
        most = max(shared)
        at = (4, 6, 7) if t == 0 else (8, 9, 10)
        row[at[0]], row[at[1]], row[at[2]] = arm, most, min(gap) if most == 0 else gap[shared.index(most)]
    row[11] = sum(max(r[1] + 1 - r[0] for r in runs[key]) for key in order if key[0] == "s")
    row[12] = int(any("UGU" in seq[r[0]:r[1]] for r in loops))
    stretch = structure[seq.find(mirnas[0]):seq.find(mirnas[0]) + len(mirnas[0])]
    row[13], row[14], row[15] = stretch.count("(") + stretch.count(")"), len(stretch), n_stem
    return row


_FEATURES_HEADER_HEAD = ("realMicRNA\trealMicRNAName\tchr\tstartPos\tendPos\tclusterName\tclusterSeq\tmajoritySeq\tstableClusterSeq\t"
                         "alignedClusterSeq\tadjustedClusterSeq\tclusterSecondSeq\ttemplateSeq\tseqCount\treadCountSum\texactMatchRatio\t"
                         "headUnstableLength\ttailUnstableLength\t")


class _writer_threads:
    """MIRGE_AMD_TABLE_THREADS for the duration of one writer call (None = leave the environment alone)."""

    def __init__(self, threads):
        self.threads, self.old = threads, None

    def __enter__(self):
        if self.threads is not None:
            self.old = os.environ.get("MIRGE_AMD_TABLE_THREADS")
            os.environ["MIRGE_AMD_TABLE_THREADS"] = str(int(self.threads))

    def __exit__(self, *exc):
        if self.threads is not None:
            if self.old is None:
                del os.environ["MIRGE_AMD_TABLE_THREADS"]
            else:
                os.environ["MIRGE_AMD_TABLE_THREADS"] = self.old


def genome_libraries(engine, genome_prefix):
    """The genome's parts resident on `engine` (bowtie.open_index's prefix resolution), added on first use:
    (library keys, FmIndex list)."""
    cache = engine.__dict__.setdefault("_predict_genomes", {})
    key = os.path.abspath(genome_prefix)
    if key not in cache:
        parts = bowtie.open_index(genome_prefix)
        keys = []
        for k, ix in enumerate(parts):
            keys.append("predict:%s:part%03d" % (key, k))
            engine.add_library(keys[-1], ix, exact_dict=False)
        cache[key] = (keys, parts)
    return cache[key]


def _check_policy(mapping_loc, seedLength, overlapLenCutoff):
    if int(mapping_loc) < 0 or int(seedLength) < 5 or int(overlapLenCutoff) < 1:
        raise ValueError("mapping_loc must be >= 0, seedLength >= 5 and overlapLenCutoff >= 1")


def _map_cluster_write(engine, rs, counts, names, seqs, genome_prefix, mapping_loc, seedLength, overlapLenCutoff, out_stem,
                       sam, timings, trim=None, remap=False, numbers=None, features=False, precursors=False, screen=False, fold=None, classifier=None,
                       report=False):
    """The body map_and_cluster and map_and_cluster_reads share: rs = the reads as a ReadSet (None: no read), names / seqs
    as write_clusters / write_sorted_sam take them; numbers: the reads' (None: read from the list `names`); classifier: what
    classifier_files returned (None: no classification); report: also the report of the classified candidates."""
    from .engine import STRATUM_ALL
    if report and classifier is None:
        raise ValueError("report needs classify: the report is built from the novel list")
    if remap and trim is None:
        raise ValueError("remap needs trim: the reads are mapped to the clusters the trim retains")
    if features and not remap:
        raise ValueError("features needs remap: the feature table is built from the rows of the second mapping")
    if precursors and not features:
        raise ValueError("precursors needs features: the windows are cut around the stable part the feature table found")
    if screen and not precursors:
        raise ValueError("screen needs precursors: the candidates it folds are the windows cut there")
    if screen and fold is None:
        raise ValueError("screen needs fold: a callable (fasta_path, str_path), or the path of RNAfold")
    if classifier is not None and not screen:
        raise ValueError("classify needs screen: the SVM reads the screened table")
    keys, parts = genome_libraries(engine, genome_prefix)
    if trim is not None:
        repeats, cutoff = trim
        if repeats is None or isinstance(repeats, (str, bytes, os.PathLike)):
            repeats = load_repeats(repeats, parts)
        if int(cutoff) < 0 or len(repeats["rep_off"]) != 1 + sum(len(ix.names) for ix in parts):
            raise ValueError("trim: the cutoff must not be negative and the repeat table must be load_repeats' over this genome")
    sam_path = out_stem + "_vs_genome_sorted.sam"
    keep = np.array(["chr" in nm for ix in parts for nm in ix.names], dtype=bool)
    if rs is not None:
        cl = engine.cluster_valid(rs, keys, counts, entry_keep=keep, threshold=int(overlapLenCutoff), strands=2,
                                  stratum_mode=STRATUM_ALL, m=int(mapping_loc), seed_len=int(seedLength), max_mm_seed=0,
                                  max_mm_total=bowtie.N_MODE_MAX_TOTAL, sorted_rows=sam, timings=timings,
                                  **({} if trim is None else {"keep_device": True}))
    else:
        cl = dict(entry=np.zeros(0, np.uint32), strand=np.zeros(0, np.uint8), start=np.zeros(0, np.uint32),
                  end=np.zeros(0, np.uint32), seq_off=np.zeros(1, np.uint64), seq=b"", count_sum=np.zeros(0, np.uint64),
                  member_off=np.zeros(1, np.uint32), members=np.zeros(0, np.uint32), suppressed=np.zeros(0, bool), n_rows=0,
                  n_valid=0, rows=tuple(np.zeros(0, dt) for dt in (np.uint32, np.int32, np.int32, np.uint8, np.uint8)))
    write_clusters(sam_path[:-4] + "_clusters.tsv", sample_name(sam_path), parts, names, cl)
    if sam:
        write_sorted_sam(sam_path, parts, names, seqs, cl["rows"], cl["suppressed"], int(mapping_loc))
    if trim is not None:
        cl["trim"] = trim_clusters(engine, cl, repeats, cutoff, out_stem, names)
        cl.pop("device", None)
        cl["trim"].pop("device", None)
        if remap:
            cl["remap"] = map_reads_to_clusters(engine, rs, numbers, counts, cl["trim"], seedLength, out_stem, names,
                                                keep_device=bool(features))
        if features:
            trimmed = dict(cl["trim"], clusters=retained_clusters(cl, cl["trim"]))
            cl["features"] = cluster_features(engine, rs, counts, trimmed, cl["remap"], parts, out_stem,
                                              **({"keep_device": True} if precursors else {}))
            if precursors:
                cl["precursors"] = cluster_precursors(engine, cl["features"], trimmed, parts, out_stem, parts_libs=keys)
                if screen:
                    cl["screen"] = screen_precursors(engine, cl["features"], cl["precursors"], fold, out_stem)
                    if classifier is not None:
                        cl["classify"] = classify_candidates(engine, cl["screen"]["path"], None, None, classifier=classifier)
                        if report:
                            cl["report"] = report_candidates(engine, cl["classify"])
                cl["features"].pop("device", None)
                cl["features"].pop("index", None)
            cl["remap"].pop("device", None)
            cl["remap"].pop("index", None)
    return cl


def map_and_cluster(engine, reads_fa, genome_prefix, mapping_loc, seedLength, overlapLenCutoff, out_stem, sam=True,
                    timings=None, trim=None, remap=False, features=False, precursors=False, screen=False, fold=None, classify=False,
                    models=None, species=None, report=False):
    """The reference's miRge2.0.py:538-548 for one reads file: bowtie `-f -n 0 -m mapping_loc -l seedLength -S -a --best`
    against the genome, samtools sort, cluster_basedon_location(<sorted.sam>, overlapLenCutoff).  Writes
    `<out_stem>_vs_genome_sorted_clusters.tsv` and (sam=True) `<out_stem>_vs_genome_sorted.sam`; returns the cluster
    arrays of Engine.cluster_valid.  mapping_loc 0 = no -m.  Nothing is written when a limit is exceeded.
    trim = (repeats, clusterSeqLenCutoff) adds :557-562 (trim_clusters: the three `_clusters_trimmed` files; the return value
    gains "trim"); repeats = load_repeats' dict over this genome, or the path of the file (None: no table).
    remap=True (needs trim) adds :566-601 (map_reads_to_clusters: `<out_stem>_vs_representative_seq_modified_selected_sorted.tsv`;
    the return value gains "remap").  features=True (needs remap) adds :604 (cluster_features: the table's `_features.tsv` and
    `_cluster.txt`; the return value gains "features").  precursors=True (needs features) adds :608 (cluster_precursors: the
    table's `_features_precusor.fa`; the return value gains "precursors").  screen=True (needs precursors and fold = a callable
    (fasta_path, str_path) or RNAfold's path) adds :610-626 (screen_precursors: two folds and the table's
    `_features_updated_stableClusterSeq_15.tsv`; the return value gains "screen").  classify=True (needs screen, models = the
    directory of miRge2.0's model files and species: human and mouse have a model of their own, every other name takes
    `others`) adds :647-648 (classify_candidates: the three filter files, `predicted_<sample>_detailed.csv` and
    `<sample>_novel_miRNAs_miRge2.0.csv`; the return value gains "classify").  The model file and the namelist are opened and
    validated before any device work.  report=True (needs classify) adds :652 without its drawing (report_candidates: the table's
    `_corrected.tsv`, `<sample>_novel_miRNAs_report.csv` and `<sample>_novel_miRNAs_report_profiles.tsv`; the return value gains
    "report")."""
    from .engine import ReadSet
    if precursors and not features:
        raise ValueError("precursors needs features: the windows are cut around the stable part the feature table found")
    if screen and not precursors:
        raise ValueError("screen needs precursors: the candidates it folds are the windows cut there")
    if classify and not screen:
        raise ValueError("classify needs screen: the SVM reads the screened table")
    if report and not classify:
        raise ValueError("report needs classify: the report is built from the novel list")
    classifier = classifier_files(models, species) if classify else None
    names, seqs = bowtie.read_fasta(reads_fa)
    longest = max((len(s) for s in seqs), default=0)
    if longest > bowtie.MAX_READ_LEN:
        raise ValueError("reads longer than %d nt are not supported; got %d" % (bowtie.MAX_READ_LEN, longest))
    _check_policy(mapping_loc, seedLength, overlapLenCutoff)
    counts = read_counts(names)
    rs = None
    if seqs:
        words, lens, nmask = pack.pack_reads(seqs, pack.words_for(max(longest, 1)))
        rs = ReadSet(words, lens, nmask, device=engine.device)
    return _map_cluster_write(engine, rs, counts, names, seqs, genome_prefix, mapping_loc, seedLength, overlapLenCutoff,
                              out_stem, sam, timings, trim, remap, features=features, precursors=precursors, screen=screen, fold=fold,
                              classifier=classifier, report=report)


def map_and_cluster_reads(engine, reads, numbers, counts, genome_prefix, mapping_loc, seedLength, overlapLenCutoff, out_stem,
                          sam=True, timings=None, trim=None, remap=False, features=False, precursors=False, screen=False, fold=None,
                          classifier=None, report=False):
    """map_and_cluster from arrays: reads = (words [W, k], lens [k], nmask [W, k] or None) of Engine.predict_gather (device
    tensors, or host arrays), numbers / counts [k] = the `mir<number>_<count>` of every read (uint32; device tensors or
    host arrays).  The same policy, files and return value as map_and_cluster on the FASTA file of those reads under those
    names; no FASTA is parsed and no Python string is made per read.  trim / remap / features / precursors / screen / fold: as
    map_and_cluster's; classifier: what classifier_files returned (None: no classification); report: as map_and_cluster's."""
    import torch
    from .engine import ReadSet
    if precursors and not features:
        raise ValueError("precursors needs features: the windows are cut around the stable part the feature table found")
    _check_policy(mapping_loc, seedLength, overlapLenCutoff)

    def host_u32(x):   # (a device tensor holds uint32 in int32 storage)
        return np.ascontiguousarray(x.cpu().numpy()).view(np.uint32) if torch.is_tensor(x) else np.ascontiguousarray(x, dtype=np.uint32)
    numbers, counts = host_u32(numbers), host_u32(counts)
    words, lens, nmask = engine._dev_reads(*reads)
    k = int(lens.shape[0])
    if numbers.shape != (k,) or counts.shape != (k,) or int(words.shape[1]) != k:
        raise ValueError("map_and_cluster_reads: words [W, k], lens, numbers and counts [k] must match")
    names = read_names(numbers, counts)
    rs, seqs = None, (b"", np.zeros(1, np.uint64))
    if k:
        lo, hi = int(lens.min()), int(lens.max())
        if hi > 32 * int(words.shape[0]):
            raise ValueError("a read of %d nt does not fit %d words" % (hi, int(words.shape[0])))
        # the batch map_and_cluster packs from the FASTA: the words the longest read needs, a mask only when an N is there
        W = pack.words_for(max(hi, 1))
        if W < int(words.shape[0]):
            words = words[:W].contiguous()
            nmask = None if nmask is None else nmask[:W].contiguous()
        if nmask is not None and not bool(nmask.any()):
            nmask = None
        rs = ReadSet.from_device(words, lens, nmask, None, lo, hi)
        if sam:
            seqs = pack.unpack_blob(words.cpu().numpy().view(np.uint64), lens.cpu().numpy(),
                                    None if nmask is None else nmask.cpu().numpy().view(np.uint64))
    return _map_cluster_write(engine, rs, counts, names, seqs, genome_prefix, mapping_loc, seedLength, overlapLenCutoff,
                              out_stem, sam, timings, trim, remap, numbers, features=features, precursors=precursors, screen=screen,
                              fold=fold, classifier=classifier, report=report)


def sample_stem(sample):
    """convert2Fasta.py:40: a sample column's name up to its first `.`."""
    return sample.strip().split(".")[0]


def _write_fasta(lib, path, words, lens, nmask, rows, extra=()):
    """mrg_write_predict_fasta: rows = (index, number, count uint32 or uint64) host arrays; extra = (sequence, number, count)
    of the reads beyond 255 nt, in file order."""
    from . import _native
    W, n = words.shape
    idx, num = (np.ascontiguousarray(a, dtype=np.uint32) for a in rows[:2])
    cnt = np.ascontiguousarray(rows[2])
    if cnt.dtype != np.uint64:
        cnt = np.ascontiguousarray(cnt, dtype=np.uint32)
    seqs = (C.c_char_p * max(len(extra), 1))(*[e[0].encode("ascii") for e in extra])
    e_num = np.array([e[1] for e in extra], dtype=np.uint64)
    e_cnt = np.array([e[2] for e in extra], dtype=np.uint64)
    got = lib.mrg_write_predict_fasta(os.fsencode(path), words.ctypes.data, W, n, lens.ctypes.data,
                                      None if nmask is None else nmask.ctypes.data, n, _ptr(idx), _ptr(num), _ptr(cnt),
                                      cnt.dtype.itemsize, idx.shape[0], seqs, _ptr(e_num), _ptr(e_cnt), len(extra))
    if got < 0:
        _native.check(int(got))
    return int(got)


def candidate_lists(engine, pass_id, lens, quant, min_len, max_len, count_cutoff, timings=None):
    """The lists of convert2Fasta.py from the arrays (Engine.predict_select once, Engine.predict_sample_reads per sample and
    list): a dict with n_raw, n_sel, the host rows (index, number, count) of `raw` and `sel` (counts uint64: the totals)
    and per sample `sample_raw[s]` and `sample_sel[s]` (counts uint32).  timings: a dict that receives `select_ms` and
    `samples_ms`, between device events (the downloads included)."""
    import torch
    ev = None
    if timings is not None:
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        ev[0].record()
    sel = engine.predict_select(pass_id, lens, quant, min_len, max_len, count_cutoff)
    quant_d = engine._dev_u32(quant)
    S = int(quant_d.shape[1]) if quant_d.dim() == 2 else 1
    total = sel["total"].cpu().numpy().view(np.uint64)
    out = dict(n_raw=sel["n_raw"], n_sel=sel["n_sel"], sample_raw=[], sample_sel=[])
    for key in ("raw", "sel"):
        no = sel[key + "_no"].cpu().numpy().view(np.uint32)
        idx = np.nonzero(no)[0].astype(np.uint32)
        out[key] = (idx, no[idx], total[idx])
    if ev:
        ev[1].record()
    for s in range(S):
        for key, thr in (("raw", 1), ("sel", int(count_cutoff))):
            rows = engine.predict_sample_reads(quant_d, sel[key + "_no"], s, thr)
            out["sample_" + key].append(tuple(t.cpu().numpy().view(np.uint32) for t in rows))
    if ev:
        ev[2].record()
        ev[2].synchronize()
        timings.update(select_ms=ev[0].elapsed_time(ev[1]), samples_ms=ev[1].elapsed_time(ev[2]))
    return out


def write_candidate_reads(outdir, sample_list, words, lens, nmask, lists, min_len, max_len, count_cutoff, long_rows=()):
    """convert2Fasta.py's files for unmapped.csv, from the arrays and the lists of candidate_lists, by the native writer
    (mrg_write_predict_fasta): unmapped_mirna.fa, unmapped_mirna_raw.fa and per sample unmapped_mirna_<stem>.fa and
    unmapped_mirna_<stem>_raw.fa in `outdir`, 2 + 2 S files (two samples with one stem share a name; the later one's file
    stays).  long_rows: (sequence, counts per sample) of the unmapped reads beyond 255 nt in the order of their rows at
    the end of unmapped.csv; their numbers continue after the packed reads'.  Returns {file name: rows}."""
    from . import _native
    lib = _native.load()
    words = np.ascontiguousarray(words, dtype=np.uint64)
    lens = np.ascontiguousarray(lens, dtype=np.uint8)
    nm = None if nmask is None else np.ascontiguousarray(nmask, dtype=np.uint64)
    raw_extra, sel_extra = [], []      # (sequence, number, total, counts)
    j, i = lists["n_raw"], lists["n_sel"]
    for seq, q in long_rows:
        q = [int(x) for x in q]
        total = sum(q)
        if total >= 1:
            j += 1
            raw_extra.append((seq, j, total, q))
        if int(min_len) <= len(seq) <= int(max_len) and total >= int(count_cutoff):
            i += 1
            sel_extra.append((seq, i, total, q))
    rows = {}
    rows["unmapped_mirna.fa"] = _write_fasta(lib, os.path.join(outdir, "unmapped_mirna.fa"), words, lens, nm, lists["sel"],
                                             [e[:3] for e in sel_extra])
    rows["unmapped_mirna_raw.fa"] = _write_fasta(lib, os.path.join(outdir, "unmapped_mirna_raw.fa"), words, lens, nm,
                                                 lists["raw"], [e[:3] for e in raw_extra])
    for key, suffix, extra, thr in (("sel", ".fa", sel_extra, int(count_cutoff)), ("raw", "_raw.fa", raw_extra, 1)):
        for s, name in enumerate(sample_list):
            fn = "unmapped_mirna_" + sample_stem(name) + suffix
            rows[fn] = _write_fasta(lib, os.path.join(outdir, fn), words, lens, nm, lists["sample_" + key][s],
                                    [(e[0], e[1], e[3][s]) for e in extra if e[3][s] >= thr])
    return rows


def clusters_main(argv):
    ap = argparse.ArgumentParser(prog="python -m mirge_amd.predict clusters")
    ap.add_argument("genome_prefix")
    ap.add_argument("reads")
    ap.add_argument("-m", dest="mapping_loc", type=int, default=3)
    ap.add_argument("-l", dest="seed_len", type=int, default=25)
    ap.add_argument("--overlap", type=int, default=14)
    ap.add_argument("-o", dest="out_stem", required=True)
    ap.add_argument("--no-sam", action="store_true")
    ap.add_argument("--trim", action="store_true", help="also write the three _clusters_trimmed files")
    ap.add_argument("--repeats", metavar="FILE", help="the repeat elements (chr, start, end, name; tab-separated) for --trim")
    ap.add_argument("-clc", dest="cluster_len_cutoff", type=int, default=30)
    ap.add_argument("--remap", action="store_true", help="with --trim: also map the reads to the retained clusters (the sorted table)")
    ap.add_argument("--features", action="store_true", help="with --remap: also build the cluster feature table (_features.tsv, _cluster.txt)")
    ap.add_argument("--precursors", action="store_true", help="with --features: also cut the precursor candidates (_features_precusor.fa)")
    ap.add_argument("--screen", action="store_true", help="with --precursors: also fold and screen the candidates "
                    "(_features_updated_stableClusterSeq_15.tsv); needs -pr or --fold-cmd")
    ap.add_argument("-pr", dest="rnafold_dir", metavar="DIR", help="the directory RNAfold is in")
    ap.add_argument("--fold-cmd", metavar="EXECUTABLE", help="the fold command itself (started as `EXECUTABLE --noPS --noLP`); overrides -pr")
    ap.add_argument("--classify", action="store_true", help="with --screen: also classify the screened candidates with the SVM "
                    "(predicted_<sample>_detailed.csv, <sample>_novel_miRNAs_miRge2.0.csv); needs --models")
    ap.add_argument("--models", metavar="DIR", help="the directory of miRge2.0's model files (<species>_svc_model.pkl, total_features_namelist.txt)")
    ap.add_argument("--report", action="store_true", help="with --classify: also the report of the novel list (the table's _corrected.tsv, "
                    "<sample>_novel_miRNAs_report.csv, <sample>_novel_miRNAs_report_profiles.tsv); the PDFs are not drawn")
    ap.add_argument("-sp", dest="species", default="human", help="the species: human and mouse have a model of their own, every other takes `others`")
    a = ap.parse_args(argv)
    if a.screen and not a.precursors:
        ap.error("--screen needs --precursors")
    if a.classify and not a.screen:
        ap.error("--classify needs --screen")
    if a.classify and not a.models:
        ap.error("--classify needs --models")
    if a.report and not a.classify:
        ap.error("--report needs --classify")
    classifier = None
    if a.classify:   # (before any device work, as -pr is checked)
        try:
            classifier = classifier_files(a.models, a.species)
        except (OSError, ValueError) as e:
            sys.stderr.write("predict clusters: %s\n" % e)
            return 1
    fold = None
    if a.screen:
        try:
            fold = resolve_fold_cmd(a.rnafold_dir, a.fold_cmd)
        except ValueError as e:
            sys.stderr.write("%s\n" % e)
            return 1
    if a.precursors and not a.features:
        ap.error("--precursors needs --features")
    if a.remap and not a.trim:
        ap.error("--remap needs --trim")
    if a.features and not a.remap:
        ap.error("--features needs --remap")
    from .engine import Engine
    try:
        eng = Engine(int(os.environ.get("MIRGE_AMD_GPU", "0")))
        try:
            cl = map_and_cluster(eng, a.reads, a.genome_prefix, a.mapping_loc, a.seed_len, a.overlap, a.out_stem,
                                 sam=not a.no_sam, trim=(a.repeats, a.cluster_len_cutoff) if a.trim else None, remap=a.remap,
                                 features=a.features, precursors=a.precursors, screen=a.screen, fold=fold, classify=a.classify,
                                 models=a.models, species=a.species, report=a.report)
        finally:
            eng.close()
    except (OSError, ValueError, MirgeAmdError) as e:
        sys.stderr.write("predict clusters: %s\n" % e)
        return 1
    sys.stderr.write("# clusters: %d from %d alignments (%d on chr entries)\n" % (len(cl["entry"]), cl["n_rows"], cl["n_valid"]))
    if a.trim:
        sys.stderr.write("# trimmed: %d of them retained\n" % cl["trim"]["n_retained"])
    if a.remap:
        sys.stderr.write("# remapped: %d reads in pass 1, %d in pass 2, %d unaligned, %d rows\n" % tuple(
            cl["remap"][k] for k in ("aligned1", "aligned2", "unaligned", "n_rows")))
    if a.features:
        sys.stderr.write("# features: %d groups, %d pass the filter, %d written (%d feature lines), %d worked out on the host\n" % tuple(
            cl["features"][k] for k in ("seen", "passed", "written", "lines", "host_groups")))
    if a.precursors:
        sys.stderr.write("# precursors: %d records, %d bytes\n" % (cl["precursors"]["records"], cl["precursors"]["bytes"]))
    if a.screen:
        sys.stderr.write("# screened: %d lines, %d candidates, %d folded again, %d worked out on the host, %d fold calls\n" % tuple(
            cl["screen"][k] for k in ("lines", "candidates", "pruned", "host_candidates", "folds")))
    if a.classify:
        sys.stderr.write("# classified: %d rows, %d after the count filter, %d with a structure, %d predicted 1, %d kept\n" % tuple(
            cl["classify"][k] for k in ("table", "dataset", "refined", "predicted", "kept")))
    if a.report:
        sys.stderr.write("# report: %d novel miRNAs from %d listed names, %d lines and %d entries worked out on the host; the PDFs are not drawn\n" % tuple(
            cl["report"][k] for k in ("entries", "listed", "host_lines", "host_entries")))
    return 0


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    if not argv or argv[0] != "clusters":
        sys.stderr.write("usage: python -m mirge_amd.predict clusters <genome_prefix> <reads.fa> [-m 3] [-l 25] [--overlap 14] "
                         "-o <out_stem> [--no-sam] [--trim [--repeats FILE] [-clc 30] [--remap [--features [--precursors [--screen -pr DIR | "
                         "--fold-cmd EXECUTABLE [--classify --models DIR [-sp SPECIES] [--report]]]]]]]\n")
        return 1
    return clusters_main(argv[1:])


if __name__ == "__main__":
    sys.exit(main())
