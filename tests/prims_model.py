"""Reference model of csrc/prims.hip in plain numpy: the three prefix sums, the segmented inclusive max-scan and the
stable radix sort over the key bits [0, bits).  Imports nothing from mirge_amd; tests/test_prims_model.py pins it against
literal Python loops on a machine without a GPU, tests/test_gpu_prims.py compares the kernels with it for equality."""
import numpy as np

_M32 = np.uint64(0xFFFFFFFF)


def inclusive_sum_u32(x):
    """out[i] = x[0] + .. + x[i] modulo 2^32."""
    x = np.asarray(x, dtype=np.uint32)
    return (np.cumsum(x, dtype=np.uint64) & _M32).astype(np.uint32)


def exclusive_sum_u64(x):
    """out[i] = x[0] + .. + x[i - 1], exact in 64 bits."""
    x = np.asarray(x, dtype=np.uint32)
    out = np.zeros(x.size, dtype=np.uint64)
    if x.size > 1:
        np.cumsum(x[:-1], dtype=np.uint64, out=out[1:])
    return out


def exclusive_sum_u32(x):
    """out[i] = x[0] + .. + x[i - 1] modulo 2^32."""
    return (exclusive_sum_u64(x) & _M32).astype(np.uint32)


def segmented_inclusive_max_u32(x, head):
    """out[i] = max of x[h .. i], h = the last index <= i with head[h] != 0; elements in front of the first head are
    segment 0 and their running maximum starts from 0.  (segment << 32) | value grows with the segment, so one running
    maximum over the packed words is the running maximum inside each segment."""
    x = np.asarray(x, dtype=np.uint32)
    head = np.asarray(head, dtype=np.uint8)
    if x.size == 0:
        return np.zeros(0, dtype=np.uint32)
    seg = np.cumsum(head != 0, dtype=np.uint64)
    packed = (seg << np.uint64(32)) | x.astype(np.uint64)
    return (np.maximum.accumulate(packed) & _M32).astype(np.uint32)


def bit_mask(bits):
    return np.uint64((1 << int(bits)) - 1)


def sort_order(keys, bits):
    """The stable permutation that sorts `keys` by their bits [0, bits)."""
    keys = np.asarray(keys)
    masked = keys.astype(np.uint64) & bit_mask(bits)
    return np.argsort(masked, kind="stable")


def radix_sort(keys, vals, bits):
    """(keys, vals) in the stable order of keys & mask(bits); the keys come out whole.  vals may be None."""
    keys = np.asarray(keys)
    order = sort_order(keys, bits)
    return keys[order], (None if vals is None else np.asarray(vals)[order])


def passes_in_second(bits):
    """Eight bits a pass, two buffers: where the result lies is the parity of ceil(bits / 8)."""
    return ((int(bits) + 7) // 8) & 1
