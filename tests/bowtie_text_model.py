"""TEST INFRASTRUCTURE: an independent writer of the bowtie front end's whole output contract (mirge_amd/bowtie.py,
INTEGRATION.md section 3), in plain Python over oracle.model's exhaustive scan.  Nothing from mirge_amd is imported.

    run(argv, parts, fasta_text) -> (stdout text, stderr text)

argv: the `bowtie` argv (options, index prefix, reads file; no output file = the text goes to stdout);
parts: list of (names, seqs), the parts of one index in order; fasta_text: the reads file's content.

Alignments: oracle.model.list_valid (bowtie_model.c) on the trimmed read (+ strand) and, without --norc, on the
reverse strand.  bowtie's `-n` seed is the read's 5' end on either strand, i.e. the LAST seed bases of the reverse
complement; list_valid puts the seed first, so the reverse strand is scanned as the complemented read against the
reversed entries (an alignment of revcomp(q) at offset o of an entry of length E is one of complement(q) at
E - o - len(q) of the reversed entry, with the same mismatches).  --best/--strata, -m, the default -k 1, the line
order and every text field are applied here.
"""
import os
import sys
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import model  # noqa: E402

_COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}
VALUED = ("--threads", "-n", "-v", "-l", "-5", "-3", "-m")


def comp(s):
    return "".join(_COMP.get(c, "N") for c in s)


def parse(argv):
    v, flags, pos = {}, set(), []
    i = 0
    while i < len(argv):
        if argv[i] in VALUED:
            v[argv[i]] = int(argv[i + 1])
            i += 2
            continue
        (flags.add if argv[i].startswith("-") else pos.append)(argv[i])
        i += 1
    if "-v" in v:
        seed = (1 << 20, v["-v"], v["-v"])
    else:
        seed = (v.get("-l", 28), v.get("-n", 2), 2)
    return dict(seed=seed, t5=v.get("-5", 0), t3=v.get("-3", 0), m=v.get("-m", 0), sam="-S" in flags,
                norc="--norc" in flags, all="-a" in flags, strata="--strata" in flags, pos=pos)


def read_fasta(text):
    names, seqs = [], []
    for line in text.splitlines():
        line = line.strip()
        if not line:
            continue
        if line[0] == ">":
            f = line[1:].split()
            names.append(f[0] if f else "")
            seqs.append("")
        elif seqs:
            seqs[-1] += "".join(c if c in "ACGT" else "N" for c in line.upper())
    return names, seqs


class World:
    def __init__(self, parts):
        self.fwd = [model.Library(n, s) for n, s in parts]
        self.rev = [model.Library(n, [x[::-1] for x in s]) for n, s in parts]
        self.names, self.seqs = [], []
        for n, s in parts:
            self.names += list(n)
            self.seqs += [x.upper() for x in s]
        self.base = [0]
        for n, _ in parts:
            self.base.append(self.base[-1] + len(n))

    def hits(self, q, seed, norc, cap):
        """[(mm, entry, offset, strand)] of every valid alignment."""
        out = []
        if not q:
            return out
        for k, lib in enumerate(self.fwd):
            out += [(mm, self.base[k] + e, o, 0) for e, o, mm in model.list_valid(lib, q, *seed, cap=cap)]
            if not norc:
                for e, o, mm in model.list_valid(self.rev[k], comp(q), *seed, cap=cap):
                    g = self.base[k] + e
                    out.append((mm, g, len(self.seqs[g]) - o - len(q), 1))
        return out


def run(argv, parts, fasta_text, cap=65536, threads=16):
    a = parse(argv)
    world = World(parts)
    names, raw = read_fasta(fasta_text)
    qs = [r[a["t5"]:len(r) - a["t3"]] if a["t3"] else r[a["t5"]:] for r in raw]
    with ThreadPoolExecutor(threads) as pool:   # (the scan is C: ctypes lets the threads run)
        found = list(pool.map(lambda q: world.hits(q, a["seed"], a["norc"], cap), qs))
    out = []
    if a["sam"]:
        out.append("@HD\tVN:1.0\tSO:unsorted\n")
        out += ["@SQ\tSN:%s\tLN:%d\n" % (n, len(s)) for n, s in zip(world.names, world.seqs)]
        out.append('@PG\tID:Bowtie\tVN:1.1.2\tCL:"%s"\n' % " ".join(["bowtie"] + list(argv)))
    n_al = n_sup = n_rep = 0
    for name, q, hs in zip(names, qs, found):
        best = min((h[0] for h in hs), default=None)
        rep = [h for h in hs if h[0] == best] if (a["strata"] or not a["all"]) else hs
        sup = bool(a["m"]) and len(rep) > a["m"]
        if sup or not rep:
            n_sup += sup
            if a["sam"]:
                out.append("%s\t4\t*\t0\t0\t*\t*\t0\t0\t%s\t%s\tXM:i:%d\n" % (name, q, "I" * len(q), a["m"] + 1 if sup else 0))
            continue
        n_al += 1
        rep.sort(key=lambda h: (h[0], -h[1], -h[2], -h[3]))
        if not a["all"]:
            rep = [min(rep)]
        for mm, e, o, st in rep:
            s = "".join(_COMP.get(c, "N") for c in reversed(q)) if st else q
            ref = world.seqs[e][o:o + len(q)]
            if a["sam"]:
                md, run_ = "", 0
                for x, y in zip(s, ref):
                    if x == y:
                        run_ += 1
                    else:
                        md += "%d%s" % (run_, y)
                        run_ = 0
                md += str(run_)
                out.append("%s\t%d\t%s\t%d\t255\t%dM\t*\t0\t0\t%s\t%s\tXA:i:%d\tMD:Z:%s\tNM:i:%d\n"
                           % (name, 16 if st else 0, world.names[e], o + 1, len(q), s, "I" * len(q), mm, md, mm))
            else:
                desc = ",".join("%d:%s>%s" % (i, y, x) for i, (x, y) in enumerate(zip(s, ref)) if x != y)
                out.append("\t".join([name, "-" if st else "+", world.names[e], str(o), s, "I" * len(q), "0", desc]) + "\n")
            n_rep += 1
    n = len(qs)

    def pct(x):
        return "%.2f%%" % (100.0 * x / n if n else 0.0)
    fail = n - n_al - n_sup
    err = ["# reads processed: %d\n" % n,
           "# reads with at least one reported alignment: %d (%s)\n" % (n_al, pct(n_al)),
           "# reads that failed to align: %d (%s)\n" % (fail, pct(fail))]
    if a["m"]:
        err.append("# reads with alignments suppressed due to -m: %d (%s)\n" % (n_sup, pct(n_sup)))
    err.append("Reported %d alignments to 1 output stream(s)\n" % n_rep)
    return "".join(out), "".join(err)


def arrays(argv, parts, fasta_text, cap=65536):
    """The model's own alignment arrays in the front end's order, for feeding mrg_write_bowtie directly:
    (names, trimmed seqs, offsets, entry, offset, strand, mm, suppressed)."""
    a = parse(argv)
    world = World(parts)
    names, raw = read_fasta(fasta_text)
    qs = [r[a["t5"]:len(r) - a["t3"]] if a["t3"] else r[a["t5"]:] for r in raw]
    offsets, rows, supp = [0], [], []
    for q in qs:
        hs = world.hits(q, a["seed"], a["norc"], cap)
        best = min((h[0] for h in hs), default=None)
        rep = [h for h in hs if h[0] == best] if (a["strata"] or not a["all"]) else hs
        sup = bool(a["m"]) and len(rep) > a["m"]
        supp.append(sup)
        if sup:
            rep = []
        rep.sort(key=lambda h: (h[0], -h[1], -h[2], -h[3]))
        if not a["all"] and rep:
            rep = [min(rep)]
        rows += rep
        offsets.append(len(rows))
    return names, qs, offsets, [r[1] for r in rows], [r[2] for r in rows], [r[3] for r in rows], \
        [r[0] for r in rows], supp
