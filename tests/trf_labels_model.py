"""CPU model of mrg_trf_assign / mrg_trf_halo (csrc/trf_labels.hip) around the numpy peaks model of
tests/trf_peaks_model.py: the backend `write_trf_samples_arrays(device_labels=True)` takes in the CPU tests, and the
yardstick of the GPU tests.  It states the definitions of include/mirge_amd.h and shares no code with
mirge_amd/trf_samples.py: a label is the root of the row's nneigh chain (the first centre on it, or -1 at a top row that
is none), not the outcome of a loop in rank order.

`forest`: (rho, rank, delta, nneigh) given by hand in place of what the passes compute, for forests no real block has.
"""
import numpy as np

from tests.trf_peaks_model import ModelPeaks

RHO_MIN, DELTA_MIN = np.float32(5.0), 8


def centres_and_labels(rho, rank, delta, nneigh):
    """One group: (centres as rows in cluster order, labels) from its rows' rho (float32), rank order, delta, nneigh."""
    n = len(rho)
    top = int(rank[0])
    d = np.asarray(delta, dtype=np.int64).copy()
    d[top] = max([0] + [int(d[i]) for i in range(n) if i != top])
    centres = [i for i in range(n) if rho[i] >= RHO_MIN and d[i] >= DELTA_MIN]
    if not centres and d.max() <= DELTA_MIN and rho.max() >= RHO_MIN:
        centres = [int(np.argmax(rho))]                       # the first row of maximal rho
    number = {row: c + 1 for c, row in enumerate(centres)}
    labels = np.zeros(n, dtype=np.int32)
    for i in range(n):
        r, steps = i, 0
        while r not in number and r != top:
            r, steps = int(nneigh[r]), steps + 1
            if not 0 <= r < n or steps > n:
                raise ValueError("nneigh leaves its group or runs in a cycle")
        labels[i] = number.get(r, -1)
    return centres, labels


class LabelsModel:
    """A ModelPeaks with rank() / assign() / labels() / border(None, ...) / halo(counts), as engine.TrfPeaks has them."""
    counts_d = None

    def __init__(self, peaks, forest=None):
        self.p = peaks
        self.off = np.asarray(peaks.off, dtype=np.int64)
        self.G, self.n = len(self.off) - 1, int(self.off[-1])
        self.max_dis = peaks.max_dis
        self._rank = self._delta = self._nneigh = self._labels = self._bord = None
        if forest is not None:
            rho, self._rank, self._delta, self._nneigh = (np.asarray(x) for x in forest)
            peaks.rho = np.asarray(rho, dtype=np.float32)          # (the border pass reads it)
        self.rho = peaks.rho
        self.forest = forest is not None

    def rank(self):
        if not self.forest:
            self._rank = np.zeros(self.n, dtype=np.uint32)
            for g in range(self.G):
                a, b = int(self.off[g]), int(self.off[g + 1])
                self._rank[a:b] = np.argsort(-self.rho[a:b], kind="stable")
        return self._rank

    def min_distance(self, rank=None):
        if not self.forest:
            self._delta, self._nneigh = self.p.min_distance(self._rank if rank is None else rank)
        return self._delta, self._nneigh

    def assign(self):
        nclust, centres, labels = np.zeros(self.G, dtype=np.uint32), [], np.zeros(self.n, dtype=np.int32)
        for g in range(self.G):
            a, b = int(self.off[g]), int(self.off[g + 1])
            if a == b:
                continue
            c, labels[a:b] = centres_and_labels(self.rho[a:b], self._rank[a:b], self._delta[a:b], self._nneigh[a:b])
            nclust[g] = len(c)
            centres += c
        self.cen_off = np.zeros(self.G + 1, dtype=np.uint32)
        self.cen_off[1:] = np.cumsum(nclust)
        self._labels, self.centers = labels, np.array(centres, dtype=np.uint32)
        return nclust, self.cen_off, self.centers

    def labels(self):
        return self._labels

    def border(self, labels, bord_off):
        self._bord_off = np.asarray(bord_off, dtype=np.int64)
        self._bord = self.p.border(self._labels if labels is None else labels, bord_off)
        return self._bord

    def halo(self, counts):
        counts = np.asarray(counts, dtype=np.uint64)
        core = np.zeros(self.n, dtype=np.uint8)
        tallies = np.zeros((len(self.centers), 4), dtype=np.uint64)
        key = np.zeros(self.n, dtype=np.int64)
        for g in range(self.G):
            a, b = int(self.off[g]), int(self.off[g + 1])
            c0, nc = int(self.cen_off[g]), int(self.cen_off[g + 1] - self.cen_off[g])
            for i in range(a, b):
                c = int(self._labels[i])
                key[i] = g * (self.n + 2) + (c - 1 if c >= 1 else nc)
                if c < 1:
                    continue                                   # no cluster: never core, in no tally
                far = self.p.D[g][i - a, int(self.centers[c0 + c - 1])] > DELTA_MIN
                dim = nc > 1 and self.rho[i] < self._bord[int(self._bord_off[g]) + c]
                core[i] = not (far or dim)
                t = tallies[c0 + c - 1]
                t[0] += 1
                t[1] += core[i]
                t[2 if core[i] else 3] += counts[i]
        return core, np.argsort(key, kind="stable").astype(np.uint32), tallies


def model_label_peaks(off, codes, nmask, span, rpm, max_len, ktab):
    """The backend of trf_samples.layout_peaks for the device_labels route."""
    return LabelsModel(ModelPeaks(off, codes, nmask, span, rpm, max_len, ktab))
