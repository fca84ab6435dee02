"""TEST INFRASTRUCTURE: the text of a `_features.tsv` plus its chromosomes as the arrays the precursor stage takes -- one
group and one retained cluster per line, the frame (H, T, head, tail) the line's columns spell out -- and what
tests/predict_precursors_model.py gives for them, laid out as mrg_predict_precursors / mrg_predict_precursor_bases leave
them.  Shared by the CPU tests of the writer and the GPU tests."""
import json
import os

import numpy as np

from tests import predict_precursors_model as model

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "predict_precursors.json")


def golden():
    with open(GOLDEN) as fh:
        return json.load(fh)


class Arrays:
    """`features` (the file's text) over `chromosomes` ({name: sequence}, in entry order)."""

    def __init__(self, features, chromosomes):
        self.chromosomes = dict(chromosomes)
        self.entries = list(chromosomes)
        rows = features.split("\n")
        head = rows[0].strip().split("\t")
        self.cnames, frames, cl = [], [], []
        for line in rows[1:]:
            if line == "":
                break
            f = line.strip().split("\t")
            name = f[5]
            parts = name.split(":")
            start, end = (int(x) for x in parts[-1][:-1].split("_")[:2])
            H, T = model.dashes(f[head.index("alignedClusterSeq")])
            hu, tu = int(f[head.index("headUnstableLength")]), int(f[head.index("tailUnstableLength")])
            self.cnames.append(name)
            frames.append((H, T, hu, -tu - 1))
            cl.append((self.entries.index(parts[2]), name[-1] == "-", start, end))
        G = len(frames)
        self.n_groups = G
        self.frame = np.array(frames, dtype=np.int32).reshape(G, 4)
        self.valid = np.ones(G, dtype=np.uint8)
        self.group_cluster = np.arange(G, dtype=np.uint32)
        self.order = np.arange(G, dtype=np.uint32)
        self.cl = dict(entry=np.array([c[0] for c in cl], dtype=np.uint32), strand=np.array([c[1] for c in cl], dtype=np.uint8),
                       start=np.array([c[2] for c in cl], dtype=np.uint32), end=np.array([c[3] for c in cl], dtype=np.uint32))
        self.entry_len = np.array([len(chromosomes[e]) for e in self.entries], dtype=np.uint32)
        recs = model.records(features, chromosomes)
        index = {n: g for g, n in enumerate(self.cnames)}
        self.rec = dict(rec_group=np.array([index[r[0]] for r in recs], dtype=np.uint32),
                        rec_lo=np.array([r[3] for r in recs], dtype=np.uint32), rec_hi=np.array([r[4] for r in recs], dtype=np.uint32),
                        rec_off=np.cumsum([0] + [len(r[5]) for r in recs]).astype(np.uint64), seq="".join(r[5] for r in recs).encode())

    def indexes(self):
        """(genome parts, cluster library) built on the host; the library's sequences are placeholders, its names count."""
        from mirge_amd.index import FmIndex
        parts = [FmIndex.build(self.entries, [self.chromosomes[e] for e in self.entries])]
        lib = None
        if self.cnames:
            lib = FmIndex.build(self.cnames, [("ACGT" * 16)[:int(e) - int(s) + 1] for s, e in zip(self.cl["start"], self.cl["end"])])
        return parts, lib
