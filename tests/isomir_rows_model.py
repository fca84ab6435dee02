"""The record and mask layout of mrg_isomir_classify (include/mirge_amd.h), written down from
mirge_amd.isomir.classify_alignment: `encode` turns that function's result into a record, `decode`
turns a record back into its result.  Shared by tests/test_isomir_native.py (the writer on the CPU)
and tests/test_gpu_isomir_gff.py (the kernel)."""
import numpy as np

from mirge_amd import isomir

REC_INTS = 8


def mask_words(W):
    return (W + 1) // 2


def encode(pre_seq, lib_seq, read, start, index_value, entry, W):
    """(rec int32 [8], mask uint64 [ceil(W / 2)]) for one alignment, from classify_alignment's own answer."""
    rec = np.zeros(REC_INTS, dtype=np.int32)
    mask = np.zeros(mask_words(W), dtype=np.uint64)
    rec[6] = entry
    res = isomir.classify_alignment(pre_seq, lib_seq, read, start, index_value)
    if res is None:
        return rec, mask
    kind, variant, pre_start, pre_end, _ = res
    snp = add = 0
    if variant != "NA":
        for item in variant.split(","):
            if item.startswith("iso_snp"):
                cls = item[len("iso_snp"):]
                snp = 1 if cls == "" else isomir.SNP_CLASSES.index(cls)
            elif item.startswith("iso_add:"):
                add, rec[3] = 1, int(item.split(":")[1])
            elif item.startswith("iso_5p:"):
                rec[2] = int(item.split(":")[1])
            elif item.startswith("iso_3p:"):
                rec[3] = int(item.split(":")[1])
            else:
                raise AssertionError(item)
    rec[0], rec[1] = pre_start, pre_end
    rec[4] = (isomir.KIND_REF if kind == "ref_miRNA" else isomir.KIND_ISOMIR) | snp << 8 | add << 16
    r0, L = pre_start - 1, len(read)
    lead = min(max(-r0, 0), L)
    trail = min(max(pre_end - len(pre_seq), 0), L - lead)
    rec[5] = lead | trail << 16
    for i, ch in enumerate(read):
        x = r0 + i
        if not (0 <= x < len(pre_seq)) or pre_seq[x] != ch:
            mask[i >> 6] |= np.uint64(1) << np.uint64(i & 63)
    return rec, mask


def cigar_text(rec, mask, read):
    lead, trail = int(rec[5]) & 0xFFFF, int(rec[5]) >> 16
    ops = []
    for i, ch in enumerate(read):
        if i < lead or i >= len(read) - trail:
            ops.append("I")
        elif (int(mask[i >> 6]) >> (i & 63)) & 1:
            ops.append(ch)
        else:
            ops.append("M")
    out, run = [], 0
    for op in ops + [None]:
        if op == "M":
            run += 1
            continue
        if run:
            out.append("M" if run == 1 else "%dM" % run)
            run = 0
        if op is not None:
            out.append(op)
    return "".join(out)


def decode(rec, mask, read):
    """classify_alignment's return value for one record: None (dropped) or (type, variant, pre_start, pre_end, cigar)."""
    kind = int(rec[4]) & 255
    if kind == isomir.KIND_DROPPED:
        return None
    assert kind in (isomir.KIND_REF, isomir.KIND_ISOMIR), "record of kind %d" % kind
    return ("ref_miRNA" if kind == isomir.KIND_REF else "isomiR", isomir.variant_text(rec), int(rec[0]), int(rec[1]),
            cigar_text(rec, mask, read))
