"""CPU model of the density-peak arrays of csrc/trf_peaks.hip (mrg_trf_rho / _delta / _border), with the
same interface as Engine.trf_peaks: the backend mirge_amd.trf_samples takes in the CPU tests, and the
yardstick of the GPU tests.

Rows are decoded from the device layout (2-bit codes, N mask, span) back to characters; distances are
getDistance's (W2C:417-449).  rho is summed left to right in double precision with np.cumsum (np.sum is
pairwise and would not match the reference's loop).
"""
import numpy as np

DASH, N_CODE = -1, 4


def decode(codes, nmask, span, rows, W):
    """Rows of the device layout -> int8 matrix [len(rows), 32 W]: 0..3 = ACGT, 4 = N, -1 = '-'."""
    rows = np.asarray(rows, dtype=np.int64)
    shifts = 2 * np.arange(32, dtype=np.uint64)
    c = ((codes[:, rows].T[:, :, None] >> shifts[None, None, :]) & np.uint64(3)).astype(np.int8).reshape(len(rows), -1)
    if nmask is not None:
        nb = ((nmask[:, rows].T[:, :, None] >> shifts[None, None, :]) & np.uint64(1)).astype(bool).reshape(len(rows), -1)
        c[nb] = N_CODE
    first = (span[rows] & 0xff).astype(np.int64)
    last = (span[rows] >> 8).astype(np.int64)
    pos = np.arange(32 * W)[None, :] + 1
    c[(pos < first[:, None]) | (pos > last[:, None])] = DASH
    return c, first, last


def distances(a, fa, la, b, fb, lb):
    """getDistance of every row of a (chars, first, last) to every row of b: int32 [len(a), len(b)]."""
    out = np.empty((len(a), len(b)), dtype=np.int32)
    bd = b != DASH
    for r0 in range(0, len(a), 32):
        x = a[r0:r0 + 32]
        sub = ((x[:, None, :] != b[None, :, :]) & (x != DASH)[:, None, :] & bd[None, :, :]).sum(axis=2)
        out[r0:r0 + 32] = (np.abs(fa[r0:r0 + 32, None] - fb[None, :]) + np.abs(la[r0:r0 + 32, None] - lb[None, :])
                           + sub)
    return out


def rho_of(drow, i, rpm, ktab):
    """local_density of row i from its distances to every row of its group (W2C:484-499)."""
    d = np.delete(drow, i)
    r = np.delete(rpm, i)
    k = np.where(d < len(ktab), ktab[np.minimum(d, len(ktab) - 1)], 0.0)
    terms = k * r                                     # each product rounded, then summed in j order
    acc = np.cumsum(terms)[-1] if len(terms) else 0.0
    return np.float32(acc + rpm[i])


class ModelPeaks:
    def __init__(self, off, codes, nmask, span, rpm, max_len, ktab):
        if max_len > 255:
            raise ValueError("templates of at most 255 nt")
        self.off = np.asarray(off, dtype=np.int64)
        self.W = (int(max_len) + 31) // 32
        self.codes, self.nmask, self.span = codes, nmask, np.asarray(span)
        self.rpm = np.asarray(rpm, dtype=np.float64)
        self.ktab = np.asarray(ktab, dtype=np.float64)
        G = len(self.off) - 1
        n = int(self.off[-1])
        self.rho = np.zeros(n, dtype=np.float32)
        self.max_dis = np.zeros(G, dtype=np.uint32)
        self.D = []
        for g in range(G):
            a, b = int(self.off[g]), int(self.off[g + 1])
            ch, f, l = decode(codes, nmask, self.span, np.arange(a, b), self.W)
            D = distances(ch, f, l, ch, f, l)
            self.D.append(D)
            for i in range(b - a):
                self.rho[a + i] = rho_of(D[i], i, self.rpm[a:b], self.ktab)
            self.max_dis[g] = D.max() if b - a > 1 else 0

    def min_distance(self, rank):
        n = int(self.off[-1])
        delta = np.zeros(n, dtype=np.int32)
        nneigh = np.zeros(n, dtype=np.int32)
        for g in range(len(self.off) - 1):
            a, b = int(self.off[g]), int(self.off[g + 1])
            rk = np.asarray(rank[a:b], dtype=np.int64)
            D = self.D[g]
            for p in range(b - a):
                i = rk[p]
                if p == 0:
                    delta[a + i], nneigh[a + i] = -1, -1
                    continue
                cand = D[i, rk[:p]]
                m = min(int(cand.min()), int(self.max_dis[g]))
                q = p - 1 - int(np.argmax(cand[::-1] == m))    # `<=` in rank order: the last of equals
                delta[a + i], nneigh[a + i] = m, rk[q]
        return delta, nneigh

    def border(self, labels, bord_off):
        bord_off = np.asarray(bord_off, dtype=np.int64)
        out = np.zeros(int(bord_off[-1]), dtype=np.float32)
        for g in range(len(self.off) - 1):
            slots = int(bord_off[g + 1] - bord_off[g])
            if slots < 3:
                continue
            a, b = int(self.off[g]), int(self.off[g + 1])
            cl = np.asarray(labels[a:b])
            rho = self.rho[a:b]
            D = self.D[g]
            for i in range(b - a):           # (pair (i, j) updates cl[j]'s slot from row j's turn)
                m = (cl != cl[i]) & (D[i] <= 3)
                if m.any():
                    v = ((rho[i] + rho[m]) / np.float32(2)).max()
                    s = int(bord_off[g]) + (int(cl[i]) if cl[i] >= 0 else int(cl[i]) + slots)
                    out[s] = max(out[s], v)
        return out


def model_peaks(off, codes, nmask, span, rpm, max_len, ktab):
    return ModelPeaks(off, codes, nmask, span, rpm, max_len, ktab)


def random_rows(rng, n, L, equal_rpm=False):
    """n rows of one template of L nt, as a report block: reads of 8..45 nt (every 7th touching the 5' end,
    every 7th + 1 the 3' end, some the whole template) with up to two substitutions or N; RPM of three decimals,
    every 5th (or all, equal_rpm) the same."""
    tmpl = "".join("ACGT"[c] for c in rng.integers(0, 4, L))
    rows = []
    for k in range(n):
        if k % 7 == 0:
            a, b = 0, min(L, int(rng.integers(8, 50)))
        elif k % 7 == 1:
            a, b = max(0, L - int(rng.integers(8, 50))), L
        elif k % 11 == 2:
            a, b = 0, L
        else:
            a = int(rng.integers(0, max(1, L - 8)))
            b = int(rng.integers(min(L, a + 8), min(L, a + 45) + 1))
        r = list(tmpl[a:b])
        for _ in range(int(rng.integers(0, 3))):
            r[int(rng.integers(0, len(r)))] = "ACGTN"[int(rng.integers(0, 5))]
        rpm = 3.25 if equal_rpm or k % 5 == 0 else float("%.3f" % rng.uniform(0.0, 60.0))
        rows.append(("-" * a + "".join(r) + "-" * (L - b), "x", 1, rpm))
    return rows
