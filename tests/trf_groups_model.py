"""CPU model of mrg_trf_sample_groups / Engine.trf_sample_groups (csrc/trf_groups.hip): the (sample, tRNA) blocks of
tRFs.samples.tmp/ stated on the arrays -- the rows of mrg_trf_classify in the order of the tsv, the packed reads, quant,
the per-sample denominators and trf.sample_tables -- with plain Python objects and no code of mirge_amd/trf_samples.py.
The `groups` backend of trf_samples.write_trf_samples_arrays in the CPU tests and the yardstick of the GPU tests.

  item         (row r, sample s) with rec[r][7] <= 2 and quant[read][s] > 0; its read is the whole read
  block        (sample, name of the entry); read_sum = the sum of its items' counts
  printed row  an item with start + len(read) <= len(template); the others count in read_sum only
  order        samples as given; blocks by (read_sum, name) descending; printed rows by (count, start, read) descending,
               the read compared as a Python string
  group        a block with a printed row; the k-th group of a sample is paired with the sample's k-th block
  row layout   span = (start + 1) | (start + len) << 8; 2-bit codes and N mask of the read at base `start` of a frame of
               ceil(max_len / 32) words, max_len = the longest template among the groups (at least 1); rpm = the RP100K
               re-read from its 3-decimal text
"""
import types

import numpy as np

KIND_DELE = 2
CODE = {"A": 0, "C": 1, "G": 2, "T": 3, "N": 0}


def read_string(words, lens, nmask, i):
    out = []
    for p in range(int(lens[i])):
        w, sh = p >> 5, 2 * (p & 31)
        if nmask is not None and (int(nmask[w, i]) >> sh) & 1:
            out.append("N")
        else:
            out.append("ACGT"[(int(words[w, i]) >> sh) & 3])
    return "".join(out)


def rp100k_text(count, denom):
    x = 100000.0 * count / denom if denom else 0.0
    return float("%.3f" % round(x, 3))


def model_groups(st, rec, words, lens, nmask, quant, denom, timings=None):
    rec = np.asarray(rec).reshape(-1, 12)
    words, quant = np.asarray(words), np.asarray(quant)
    quant = quant.reshape(words.shape[1], -1)
    S = quant.shape[1]
    entries = np.asarray(st.entries)
    g = types.SimpleNamespace(no_template_row=None, n_items=0, filled=False)
    per_sample = [dict() for _ in range(S)]            # name id -> items (read string, r, entry, start, type, count)
    strings = {}
    for r, row in enumerate(rec.tolist()):
        if row[7] > KIND_DELE:
            continue
        read, entry, start = row[0], row[1], row[2]
        for s in range(S):
            count = int(quant[read, s])
            if count == 0:
                continue
            g.n_items += 1
            if entries[entry, 1] < 0 and g.no_template_row is None:
                g.no_template_row = r
            if read not in strings:
                strings[read] = read_string(words, lens, nmask, read)
            per_sample[s].setdefault(int(entries[entry, 0]), []).append((count, start, strings[read], r, entry, row[4]))
    blocks, sums, groups, off, rows = [], [], [], [0], []
    for s in range(S):
        order = sorted(((sum(i[0] for i in items), st.names[name], name) for name, items in per_sample[s].items()),
                       reverse=True)
        first_block, k = len(blocks), 0
        for read_sum, _, name in order:
            items = per_sample[s][name]
            rep = min(i[4] for i in items)
            tlen = int(entries[rep, 1])
            printed = sorted((i for i in items if i[1] + len(i[2]) <= tlen), reverse=True)
            blocks.append([s, rep, len(rows), len(printed), len(groups) if printed else -1, 0])
            sums.append(read_sum)
            if printed:
                groups.append([len(blocks) - 1, first_block + k])
                k += 1
                rows += [(s, i) for i in printed]
                off.append(len(rows))
    g.blocks = np.array(blocks, dtype=np.int32).reshape(-1, 6)
    g.block_sums = np.array(sums, dtype=np.uint64)
    g.groups = np.array(groups, dtype=np.int32).reshape(-1, 2)
    g.off = np.array(off, dtype=np.uint32)
    g.G, g.n = len(groups), len(rows)
    g.max_len = max([int(entries[g.blocks[b, 1], 1]) for b, _ in groups] + [1])
    g.has_n = any("N" in i[2] for _, i in rows)
    g.rows = np.array([(i[3], i[0], i[5]) for _, i in rows], dtype=np.uint32).reshape(-1, 3)
    if g.no_template_row is not None or g.max_len > 255:
        return g
    g.filled = True
    W = (g.max_len + 31) // 32
    codes = [[0] * g.n for _ in range(W)]
    nm = [[0] * g.n for _ in range(W)]
    g.span = np.zeros(g.n, dtype=np.uint16)
    g.rpm = np.zeros(g.n, dtype=np.float64)
    for at, (s, (count, start, read, _, _, _)) in enumerate(rows):
        for i, ch in enumerate(read):
            p = start + i
            codes[p >> 5][at] |= CODE[ch] << (2 * (p & 31))
            if ch == "N":
                nm[p >> 5][at] |= 1 << (2 * (p & 31))
        g.span[at] = (start + 1) | ((start + len(read)) << 8)
        g.rpm[at] = rp100k_text(count, int(denom[s]))
    g.codes = np.array(codes, dtype=np.uint64).reshape(W, g.n)
    g.nmask = np.array(nm, dtype=np.uint64).reshape(W, g.n) if g.has_n else None
    return g
