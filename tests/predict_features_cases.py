"""TEST INFRASTRUCTURE: a table text of predict mode's second mapping plus its chromosomes as the arrays the feature stage
takes -- the reads, the retained clusters, the rows in file order -- and the numbers tests/predict_features_model.py gives
for them, laid out as mrg_predict_feature_groups / _align / _tally / _neighbors leave them.  Shared by the CPU tests of the
writer and the GPU tests."""
import json
import os

import numpy as np

from tests import predict_features_model as model
from tests import predict_remap_model as prm

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "predict_features.json")
STATE = {"Null": 0, "Good": 1, "Bad": 2}


def golden_worlds():
    with open(GOLDEN) as fh:
        return json.load(fh)["worlds"]


class Arrays:
    """The table `text` over `chromosomes` ({name: sequence}, in entry order) as arrays."""

    def __init__(self, text, chromosomes):
        self.chromosomes = dict(chromosomes)
        self.entries = list(chromosomes)
        reads, clusters = {}, {}
        self.names, self.seqs, self.cnames, self.cseqs, rows = [], [], [], [], []
        for line in text.splitlines():
            f = line.split("\t")
            if f[0] not in reads:
                reads[f[0]] = len(self.names)
                self.names.append(f[0])
                self.seqs.append(f[2])
            if f[5] not in clusters:
                clusters[f[5]] = len(self.cnames)
                self.cnames.append(f[5])
                self.cseqs.append(f[3])
            rows.append((reads[f[0]], clusters[f[5]]))
        self.counts = np.array([int(n.split("_")[-1]) for n in self.names], dtype=np.uint32)
        self.numbers = np.array([prm.read_number(n) for n in self.names], dtype=np.uint32)
        self.row_read = np.array([r for r, _ in rows], dtype=np.uint32)
        self.row_cluster = np.array([c for _, c in rows], dtype=np.uint32)
        fields = [model.name_fields(n) for n in self.cnames]
        self.cl = dict(entry=np.array([self.entries.index(f[0]) for f in fields], dtype=np.uint32),
                       strand=np.array([f[3] == "-" for f in fields], dtype=np.uint8),
                       start=np.array([f[1] for f in fields], dtype=np.uint32), end=np.array([f[2] for f in fields], dtype=np.uint32))
        self.kept = np.array([prm.cluster_number(n) - 1 for n in self.cnames], dtype=np.uint32)
        self.kept_seq_off = np.zeros(len(self.cseqs) + 1, dtype=np.uint64)
        np.cumsum([len(s) for s in self.cseqs], out=self.kept_seq_off[1:])
        self.kept_orig = "".join(self.cseqs).encode()
        self.entry_len = np.array([len(chromosomes[e]) for e in self.entries], dtype=np.uint32)
        self.entry_rank = np.zeros(len(self.entries), dtype=np.uint32)
        for k, e in enumerate(sorted(self.entries)):
            self.entry_rank[self.entries.index(e)] = k
        # the groups: runs of equal cluster in file order
        starts = [t for t in range(len(rows)) if t == 0 or rows[t][1] != rows[t - 1][1]]
        self.group_off = np.array(starts + [len(rows)], dtype=np.uint32)
        self.group_cluster = self.row_cluster[self.group_off[:-1].astype(np.int64)] if rows else np.zeros(0, np.uint32)
        self.n_groups = len(starts)
        self.row_group = np.zeros(len(rows), dtype=np.uint32)
        for g in range(self.n_groups):
            self.row_group[self.group_off[g]:self.group_off[g + 1]] = g

    def packed(self):
        from mirge_amd import pack
        if not self.seqs:
            return np.zeros((1, 0), np.uint64), np.zeros(0, np.uint8), None
        return pack.pack_reads(self.seqs)

    def expected(self, text, align=None):
        """The model's numbers per group, as the device calls leave them: a dict of arrays [G] plus order, rows_text
        {g: the frame as text} and the model's info."""
        _, _, info = model.run(text, self.chromosomes, "x.tsv", align)
        G = self.n_groups
        by_name = {self.cnames[int(c)]: g for g, c in enumerate(self.group_cluster)}
        out = dict(group_sum=np.zeros(G, np.uint64), group_pass=np.zeros(G, np.uint8), valid=np.zeros(G, np.uint8),
                   frame=np.zeros((G, 4), np.int32), exact=np.zeros(G, np.uint64), nine=np.zeros((G, 45), np.uint64),
                   nb_t=np.zeros(G, np.uint32), nb_up=np.zeros(G, np.int64), nb_down=np.zeros(G, np.int64), nb_flags=np.zeros(G, np.uint8),
                   row_diag=np.zeros(len(self.row_read), np.int32), row_ident=np.zeros(len(self.row_read), np.uint8))
        for g in range(G):
            members = self.row_read[self.group_off[g]:self.group_off[g + 1]].astype(np.int64)
            out["group_sum"][g] = int(self.counts[members].astype(np.uint64).sum())
        order, rows_text = [], {}
        for d in info["groups"]:
            g = by_name[d["cluster"]]
            out["group_pass"][g] = 1
            rows_text[g] = "\n".join(d["rows"])
            lo = int(self.group_off[g])
            for m, row in enumerate(d["rows"][1:]):
                out["row_diag"][lo + m] = (len(row) - len(row.lstrip("-"))) - d["H"]
                out["row_ident"][lo + m] = model.identity(d["rows"][0], row)
            if d["head"] is None:
                out["frame"][g] = (d["H"], d["T"], 0, 0)
                continue
            out["valid"][g] = 1
            out["frame"][g] = (d["H"], d["T"], d["head"], d["tail"])
            out["exact"][g] = d["exact"]
            out["nine"][g] = d["nine"]
            out["nb_t"][g] = d["t"]
            out["nb_up"][g] = d["up"] or 0
            out["nb_down"][g] = d["down"] or 0
            out["nb_flags"][g] = (1 if d["up"] is None else 0) | (2 if d["down"] is None else 0) | (STATE[d["state"]] << 2)
            order.append(g)
        out["order"] = np.array(order, dtype=np.uint32)
        out["rows_text"] = rows_text
        out["info"] = info
        return out

    def indexes(self):
        """(genome parts, cluster library) built on the host."""
        from mirge_amd.index import FmIndex
        parts = [FmIndex.build(self.entries, [self.chromosomes[e] for e in self.entries])]
        return parts, (FmIndex.build(self.cnames, self.cseqs) if self.cnames else None)
