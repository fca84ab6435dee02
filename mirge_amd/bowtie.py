"""A bowtie-compatible front end, so that the unmodified miRge2.0 runs on this engine (`-pb <dir>`).

miRge2.0 reaches its aligner only through `os.system("<-pb dir>/bowtie ...")`, `bowtie-build` and
`bowtie-inspect`.  `python -m mirge_amd.bowtie install <dir>` writes those three programs; each calls one of

    python -m mirge_amd.bowtie align   <bowtie options> <index prefix> <reads.fa> [<out>]
    python -m mirge_amd.bowtie build   [-f] <in.fa> <prefix>          (writes <prefix>.mrgfm)
    python -m mirge_amd.bowtie inspect [-n] <prefix>

`align` accepts exactly the options the reference passes (see OPTIONS below and INTEGRATION.md section 3); the
alignments come from the GPU (Engine.list_valid = mrg_list_valid_count / _fill; reads beyond 255 nt:
Engine.list_valid_long = mrg_list_valid_long_count / _fill) and the text from mrg_write_bowtie.
The device is $MIRGE_AMD_GPU (default 0); $MIRGE_AMD_LONG_READS=1 admits reads beyond 255 nt, which `align` refuses
otherwise.
"""
import collections
import ctypes as C
import os
import sys

import numpy as np

from . import pack
from ._native import MirgeAmdError

USAGE = ("usage: bowtie [--threads N] [--phred64-quals] [-f] [-S] [-n N | -v V] [-l L] [-5 N] [-3 N] [-a] [--best] "
         "[--strata] [-m M] [--norc] <index prefix> <reads.fa> [<out>]")
MAX_READ_LEN = 255      # the packed listing's bound (one length byte); longer reads take the ragged listing,
LONG_READS_ENV = "MIRGE_AMD_LONG_READS"   # ... when this is 1 in the environment (miRge2.0 fixes bowtie's argv); else exit 1
V_MODE_SEED = 1024      # `-v`: the whole read is seed (engine.V_MODE_SEED)
DEFAULT_SEED_LEN = 28   # bowtie's -l default
N_MODE_MAX_TOTAL = 2    # -e 70 at the rounded FASTA quality 30
# options that take a value, and the flags
OPTIONS = {"--threads": int, "-n": int, "-v": int, "-l": int, "-5": int, "-3": int, "-m": int}
FLAGS = ("--phred64-quals", "-f", "-S", "-a", "--best", "--strata", "--norc")

Align = collections.namedtuple("Align", "mode mm seed trims strands stratum_mode m sam k1 index reads out")


class UsageError(ValueError):
    pass


def parse_align(argv):
    """bowtie argv -> Align(mode 'n'/'v', mm, seed (seed_len, max_mm_seed, max_mm_total), trims (5', 3'),
    strands 1/2, stratum_mode 'best'/'all', m (0 = none), sam, k1 (no -a: one alignment per read), index, reads,
    out (None = standard output)).  Raises UsageError."""
    vals, flags, pos = {}, set(), []
    i = 0
    while i < len(argv):
        a = argv[i]
        if a in OPTIONS:
            if i + 1 >= len(argv):
                raise UsageError("option %s needs a value" % a)
            try:
                vals[a] = OPTIONS[a](argv[i + 1])
            except ValueError:
                raise UsageError("bad value for %s: %r" % (a, argv[i + 1]))
            i += 2
            continue
        if a in FLAGS:
            flags.add(a)
        elif a.startswith("-") and a != "-":
            raise UsageError("unsupported option %s" % a)
        else:
            pos.append(a)
        i += 1
    if len(pos) not in (2, 3):
        raise UsageError("expected <index prefix> <reads.fa> [<out>]")
    if "-f" not in flags:
        raise UsageError("only FASTA reads (-f) are supported")
    if "-n" in vals and "-v" in vals:
        raise UsageError("-n and -v are exclusive")
    if "-v" in vals:
        mode, mm = "v", vals["-v"]
        if not 0 <= mm <= 3:
            raise UsageError("-v must be 0..3")
        seed = (V_MODE_SEED, mm, mm)
    else:
        mode, mm = "n", vals.get("-n", 2)
        if not 0 <= mm <= 2:
            raise UsageError("-n must be 0..2")
        seed_len = vals.get("-l", DEFAULT_SEED_LEN)
        if seed_len < 5:
            raise UsageError("-l must be at least 5")
        seed = (seed_len, mm, N_MODE_MAX_TOTAL)
    trims = (vals.get("-5", 0), vals.get("-3", 0))
    if min(trims) < 0 or vals.get("-m", 1) < 1:
        raise UsageError("-5 / -3 must be >= 0 and -m >= 1")
    all_ = "-a" in flags
    stratum = "best" if (not all_ or "--strata" in flags) else "all"
    return Align(mode, mm, seed, trims, 1 if "--norc" in flags else 2, stratum, vals.get("-m", 0), "-S" in flags,
                 not all_, pos[0], pos[1], pos[2] if len(pos) == 3 else None)


def read_fasta(path):
    """(names up to the first whitespace, sequences upper-case with every non-ACGT letter as N), file order."""
    names, seqs, cur = [], [], None
    table = bytes.maketrans(b"acgtn", b"ACGTN")
    with open(path, "rb") as fh:
        for line in fh:
            line = line.strip()
            if not line:
                continue
            if line[:1] == b">":
                if cur is not None:
                    seqs.append(b"".join(cur))
                parts = line[1:].split()
                names.append(parts[0].decode() if parts else "")
                cur = []
            elif cur is not None:
                cur.append(line.translate(table))
    if cur is not None:
        seqs.append(b"".join(cur))
    out = []
    for s in seqs:
        s = s.decode("ascii", "replace")
        if s.strip("ACGT"):
            s = "".join(ch if ch in "ACGT" else "N" for ch in s)
        out.append(s)
    return names, out


def trim(seq, t5, t3):
    return seq[t5:len(seq) - t3] if t3 else seq[t5:]


def open_index(prefix):
    """The index prefix as cli.py resolves it: `.mrgfm`, `.fa` / `.fasta`, the reference's `.1.ebwt`, else every
    `.partNNN.mrgfm` (the parts of one genome).  Returns a list of FmIndex."""
    from .index import FmIndex
    if any(os.path.isfile(prefix + e) for e in (".mrgfm", ".fa", ".fasta", ".1.ebwt")):
        return [FmIndex.open_prefix(prefix)]
    return FmIndex.open_prefix_parts(prefix)


def _blob(strs):
    b = [s.encode() for s in strs]
    off = np.zeros(len(b) + 1, dtype=np.uint64)
    np.cumsum([len(x) for x in b], out=off[1:])
    return b"".join(b), off


def write_bowtie(out, sam, cmdline, parts, names, seqs, offsets, entry, offset, strand, mm, suppressed, m):
    """mrg_write_bowtie over host arrays (out None = standard output).  Returns the summary dict."""
    from . import _native
    lib = _native.load()
    nb, no = _blob(names)
    sb, so = _blob(seqs)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    entry = np.ascontiguousarray(entry, dtype=np.int32)
    offset = np.ascontiguousarray(offset, dtype=np.int32)
    strand = np.ascontiguousarray(strand, dtype=np.uint8)
    mm = np.ascontiguousarray(mm, dtype=np.uint8)
    supp = np.ascontiguousarray(suppressed, dtype=np.uint8)
    hs = (C.c_void_p * max(len(parts), 1))(*[p._h.value for p in parts])
    summary = np.zeros(4, dtype=np.uint64)
    if out is None:
        sys.stdout.flush()
    _native.check(lib.mrg_write_bowtie(
        None if out is None else os.fsencode(out), 1 if sam else 0, cmdline.encode(), hs, len(parts), len(names), nb,
        no.ctypes.data, sb, so.ctypes.data, offsets.ctypes.data, entry.ctypes.data, offset.ctypes.data, strand.ctypes.data,
        mm.ctypes.data, supp.ctypes.data, int(m), summary.ctypes.data))
    return dict(processed=int(summary[0]), aligned=int(summary[1]), suppressed=int(summary[2]), reported=int(summary[3]))


def summary_text(s, with_m):
    """bowtie's stderr summary (parseBowtieLog reads the first two lines, RAP:9-18)."""
    n = s["processed"]

    def pct(x):
        return "%.2f%%" % (100.0 * x / n if n else 0.0)
    failed = n - s["aligned"] - s["suppressed"]
    lines = ["# reads processed: %d" % n,
             "# reads with at least one reported alignment: %d (%s)" % (s["aligned"], pct(s["aligned"])),
             "# reads that failed to align: %d (%s)" % (failed, pct(failed))]
    if with_m:
        lines.append("# reads with alignments suppressed due to -m: %d (%s)" % (s["suppressed"], pct(s["suppressed"])))
    lines.append("Reported %d alignments to 1 output stream(s)" % s["reported"])
    return "\n".join(lines) + "\n"


def keep_one(offsets, arrays):
    """bowtie's default -k 1: the last listed alignment of each read (lists are ordered so that it is the lowest
    (mm, entry, offset, strand) of the best stratum)."""
    has = offsets[1:] > offsets[:-1]
    pick = offsets[1:][has] - 1
    new_off = np.zeros_like(offsets)
    np.cumsum(has, out=new_off[1:])
    return new_off, [a[pick] for a in arrays]


def merge_listings(n, idx_a, listing_a, idx_b, listing_b):
    """Two listings (offsets[k+1], entry, offset, strand, mm, suppressed[k]: Engine.list_valid's tuple) of disjoint
    subsets of n reads, read i of listing x being read idx_x[i] of the file, as ONE listing in file order: every read's
    rows unchanged and in their order.  A read in neither subset has no rows and is not suppressed."""
    counts = np.zeros(n, dtype=np.int64)
    supp = np.zeros(n, dtype=bool)
    for idx, lst in ((idx_a, listing_a), (idx_b, listing_b)):
        idx = np.asarray(idx, dtype=np.int64)
        counts[idx] = np.diff(np.asarray(lst[0], dtype=np.int64))
        supp[idx] = np.asarray(lst[5], dtype=bool)
    offsets = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(counts, out=offsets[1:])
    total = int(offsets[n])
    rows = [np.zeros(total, dtype=dt) for dt in (np.int32, np.int32, np.uint8, np.uint8)]
    for idx, lst in ((idx_a, listing_a), (idx_b, listing_b)):
        idx = np.asarray(idx, dtype=np.int64)
        src = np.asarray(lst[0], dtype=np.int64)
        k = np.diff(src)
        # row t of the listing, t in [src[i], src[i + 1]), goes to offsets[idx[i]] + (t - src[i])
        to = np.repeat(offsets[idx] - src[:-1], k) + np.arange(int(src[-1]) if len(src) else 0, dtype=np.int64)
        for dst, a in zip(rows, lst[1:5]):
            dst[to] = np.asarray(a)[:len(to)]
    return (offsets,) + tuple(rows) + (supp,)


def align(opt, cmdline, device=None):
    from .engine import Engine, ReadSet, STRATUM_ALL, STRATUM_BEST
    names, raw = read_fasta(opt.reads)
    seqs = [trim(s, *opt.trims) for s in raw]
    lens = np.fromiter((len(s) for s in seqs), dtype=np.int64, count=len(seqs))
    # what one length byte describes goes through the packed listing, in one call; the rest through the ragged one
    short, long_ = np.nonzero(lens <= MAX_READ_LEN)[0], np.nonzero(lens > MAX_READ_LEN)[0]
    if len(long_) and os.environ.get(LONG_READS_ENV, "0") != "1":
        raise UsageError("reads longer than %d nt (after -5/-3) are not supported unless %s=1 is set (it lists them with the "
                         "wave-per-read kernel); got %d" % (MAX_READ_LEN, LONG_READS_ENV, int(lens.max())))
    parts = open_index(opt.index)
    dev = int(os.environ.get("MIRGE_AMD_GPU", "0")) if device is None else int(device)
    eng = Engine(dev)
    try:
        keys = []
        for k, ix in enumerate(parts):
            keys.append("part%03d" % k)
            eng.add_library(keys[-1], ix, exact_dict=False)
        n = len(seqs)
        seed_len, mm_seed, mm_total = opt.seed
        how = dict(strands=opt.strands, stratum_mode=STRATUM_BEST if opt.stratum_mode == "best" else STRATUM_ALL, m=opt.m,
                   max_mm_seed=mm_seed, max_mm_total=mm_total)
        empty = (np.zeros(1, dtype=np.int64), np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.uint8),
                 np.zeros(0, np.uint8), np.zeros(0, bool))
        listing = empty
        if len(short):
            sub = seqs if not len(long_) else [seqs[i] for i in short]
            words, lens8, nmask = pack.pack_reads(sub, pack.words_for(max(int(lens[short].max()), 1)))
            listing = eng.list_valid(ReadSet(words, lens8, nmask, device=eng.device), keys, seed_len=seed_len, **how)
        if len(long_):
            # (`-v`: the whole read is seed, however long it is)
            long_seed = max(seed_len, int(lens.max())) if opt.mode == "v" else seed_len
            listing = merge_listings(n, short, listing, long_,
                                     eng.list_valid_long([seqs[i] for i in long_], keys, seed_len=long_seed, **how))
        off, entry, offset, strand, mm, supp = listing
        if opt.k1:
            off, (entry, offset, strand, mm) = keep_one(off, (entry, offset, strand, mm))
        s = write_bowtie(opt.out, opt.sam, cmdline, parts, names, seqs, off, entry, offset, strand, mm, supp, opt.m)
    finally:
        eng.close()
    return s


def align_main(argv):
    try:
        opt = parse_align(argv)
    except UsageError as e:
        sys.stderr.write("bowtie: %s\n%s\n" % (e, USAGE))
        return 1
    try:
        s = align(opt, "bowtie " + " ".join(argv))
    except UsageError as e:
        sys.stderr.write("bowtie: %s\n" % e)
        return 1
    except (OSError, MirgeAmdError) as e:
        sys.stderr.write("bowtie: %s\n" % e)
        return 1
    sys.stdout.flush()
    sys.stderr.write(summary_text(s, opt.m > 0))
    return 0


def build_main(argv):
    args = [a for a in argv if a != "-f"]
    if len(args) != 2 or any(a.startswith("-") for a in args):
        sys.stderr.write("usage: bowtie-build [-f] <in.fa> <prefix>\n")
        return 1
    from .index import FmIndex
    try:
        # MIRGE_AMD_BUILD_GPU=<id>: sort the suffixes on that GPU (a failure there is an error, not a reason to
        # fall back to the host builder)
        gpu = os.environ.get("MIRGE_AMD_BUILD_GPU")
        FmIndex.from_fasta(args[0], device=int(gpu) if gpu else None).save(args[1] + ".mrgfm")
    except (OSError, ValueError, MirgeAmdError) as e:
        sys.stderr.write("bowtie-build: %s\n" % e)
        return 1
    return 0


def inspect_main(argv):
    names_only = "-n" in argv
    args = [a for a in argv if a != "-n"]
    if len(args) != 1 or args[0].startswith("-"):
        sys.stderr.write("usage: bowtie-inspect [-n] <prefix>\n")
        return 1
    try:
        parts = open_index(args[0])
    except (OSError, MirgeAmdError) as e:
        sys.stderr.write("bowtie-inspect: %s\n" % e)
        return 1
    out = sys.stdout
    for ix in parts:
        for i, name in enumerate(ix.names):
            out.write(name + "\n" if names_only else ">%s\n%s\n" % (name, ix.sequence(i)))
    out.flush()
    return 0


_SCRIPT = """#!%(python)s
# written by `python -m mirge_amd.bowtie install`: miRge2.0's %(prog)s, answered by mirge_amd
import sys
sys.path.insert(0, %(root)r)
from mirge_amd import bowtie
sys.exit(bowtie.%(fn)s(sys.argv[1:]))
"""
PROGRAMS = {"bowtie": "align_main", "bowtie-build": "build_main", "bowtie-inspect": "inspect_main"}


def install_main(argv):
    if len(argv) != 1:
        sys.stderr.write("usage: python -m mirge_amd.bowtie install <dir>\n")
        return 1
    d = argv[0]
    os.makedirs(d, exist_ok=True)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for prog, fn in PROGRAMS.items():
        path = os.path.join(d, prog)
        with open(path, "w") as fh:
            fh.write(_SCRIPT % dict(python=sys.executable, prog=prog, root=root, fn=fn))
        os.chmod(path, 0o755)
    return 0


COMMANDS = {"align": align_main, "build": build_main, "inspect": inspect_main, "install": install_main}


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    if not argv or argv[0] not in COMMANDS:
        sys.stderr.write("usage: python -m mirge_amd.bowtie {align,build,inspect,install} ...\n")
        return 1
    return COMMANDS[argv[0]](argv[1:])


if __name__ == "__main__":
    sys.exit(main())
