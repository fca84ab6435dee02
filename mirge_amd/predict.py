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


def write_clusters(path, sample, parts, names, cl, threads=None):
    """mrg_write_clusters over the arrays of Engine.cluster_valid (parts: the FmIndex list; names: the reads')."""
    from . import _native
    lib = _native.load()
    nb, no = bowtie._blob(names)
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
            arr["member_off"].ctypes.data, _ptr(arr["members"]), len(names), nb, no.ctypes.data, C.byref(rows)))
    return int(rows.value)


def write_sorted_sam(path, parts, names, seqs, rows, suppressed, m, threads=None):
    """mrg_write_sorted_sam: rows = (read, entry, offset, strand, mm) in the order to print."""
    from . import _native
    lib = _native.load()
    nb, no = bowtie._blob(names)
    sb, so = bowtie._blob(seqs)
    hs = (C.c_void_p * max(len(parts), 1))(*[p._h.value for p in parts])
    read, entry, offset, strand, mm = (np.ascontiguousarray(a, dtype=dt) for a, dt in
                                       zip(rows, (np.uint32, np.int32, np.int32, np.uint8, np.uint8)))
    supp = np.ascontiguousarray(suppressed, dtype=np.uint8)
    summary = np.zeros(4, dtype=np.uint64)
    with _writer_threads(threads):
        _native.check(lib.mrg_write_sorted_sam(
            os.fsencode(path), hs, len(parts), len(names), nb, no.ctypes.data, sb, so.ctypes.data, len(read), _ptr(read),
            _ptr(entry), _ptr(offset), _ptr(strand), _ptr(mm), _ptr(supp), int(m), summary.ctypes.data))
    return dict(processed=int(summary[0]), aligned=int(summary[1]), suppressed=int(summary[2]), reported=int(summary[3]))


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


def map_and_cluster(engine, reads_fa, genome_prefix, mapping_loc, seedLength, overlapLenCutoff, out_stem, sam=True,
                    timings=None):
    """The reference's miRge2.0.py:538-548 for one reads file: bowtie `-f -n 0 -m mapping_loc -l seedLength -S -a --best`
    against the genome, samtools sort, cluster_basedon_location(<sorted.sam>, overlapLenCutoff).  Writes
    `<out_stem>_vs_genome_sorted_clusters.tsv` and (sam=True) `<out_stem>_vs_genome_sorted.sam`; returns the cluster
    arrays of Engine.cluster_valid.  mapping_loc 0 = no -m.  Nothing is written when a limit is exceeded."""
    from .engine import ReadSet, STRATUM_ALL
    names, seqs = bowtie.read_fasta(reads_fa)
    longest = max((len(s) for s in seqs), default=0)
    if longest > bowtie.MAX_READ_LEN:
        raise ValueError("reads longer than %d nt are not supported; got %d" % (bowtie.MAX_READ_LEN, longest))
    if int(mapping_loc) < 0 or int(seedLength) < 5 or int(overlapLenCutoff) < 1:
        raise ValueError("mapping_loc must be >= 0, seedLength >= 5 and overlapLenCutoff >= 1")
    counts = read_counts(names)
    keys, parts = genome_libraries(engine, genome_prefix)
    sam_path = out_stem + "_vs_genome_sorted.sam"
    keep = np.array(["chr" in nm for ix in parts for nm in ix.names], dtype=bool)
    if seqs:
        words, lens, nmask = pack.pack_reads(seqs, pack.words_for(max(longest, 1)))
        rs = ReadSet(words, lens, nmask, device=engine.device)
        cl = engine.cluster_valid(rs, keys, counts, entry_keep=keep, threshold=int(overlapLenCutoff), strands=2,
                                  stratum_mode=STRATUM_ALL, m=int(mapping_loc), seed_len=int(seedLength), max_mm_seed=0,
                                  max_mm_total=bowtie.N_MODE_MAX_TOTAL, sorted_rows=sam, timings=timings)
    else:
        cl = dict(entry=np.zeros(0, np.uint32), strand=np.zeros(0, np.uint8), start=np.zeros(0, np.uint32),
                  end=np.zeros(0, np.uint32), seq_off=np.zeros(1, np.uint64), seq=b"", count_sum=np.zeros(0, np.uint64),
                  member_off=np.zeros(1, np.uint32), members=np.zeros(0, np.uint32), suppressed=np.zeros(0, bool), n_rows=0,
                  n_valid=0, rows=tuple(np.zeros(0, dt) for dt in (np.uint32, np.int32, np.int32, np.uint8, np.uint8)))
    write_clusters(sam_path[:-4] + "_clusters.tsv", sample_name(sam_path), parts, names, cl)
    if sam:
        write_sorted_sam(sam_path, parts, names, seqs, cl["rows"], cl["suppressed"], int(mapping_loc))
    return cl


def clusters_main(argv):
    ap = argparse.ArgumentParser(prog="python -m mirge_amd.predict clusters")
    ap.add_argument("genome_prefix")
    ap.add_argument("reads")
    ap.add_argument("-m", dest="mapping_loc", type=int, default=3)
    ap.add_argument("-l", dest="seed_len", type=int, default=25)
    ap.add_argument("--overlap", type=int, default=14)
    ap.add_argument("-o", dest="out_stem", required=True)
    ap.add_argument("--no-sam", action="store_true")
    a = ap.parse_args(argv)
    from .engine import Engine
    try:
        eng = Engine(int(os.environ.get("MIRGE_AMD_GPU", "0")))
        try:
            cl = map_and_cluster(eng, a.reads, a.genome_prefix, a.mapping_loc, a.seed_len, a.overlap, a.out_stem,
                                 sam=not a.no_sam)
        finally:
            eng.close()
    except (OSError, ValueError, MirgeAmdError) as e:
        sys.stderr.write("predict clusters: %s\n" % e)
        return 1
    sys.stderr.write("# clusters: %d from %d alignments (%d on chr entries)\n" % (len(cl["entry"]), cl["n_rows"], cl["n_valid"]))
    return 0


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    if not argv or argv[0] != "clusters":
        sys.stderr.write("usage: python -m mirge_amd.predict clusters <genome_prefix> <reads.fa> [-m 3] [-l 25] [--overlap 14] "
                         "-o <out_stem> [--no-sam]\n")
        return 1
    return clusters_main(argv[1:])


if __name__ == "__main__":
    sys.exit(main())
