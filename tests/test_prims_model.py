"""The numpy model of the device primitives (tests/prims_model.py) against literal Python loops, on the CPU: a few
hundred small random cases and the worked bits = 4 example.  tests/test_gpu_prims.py trusts the model; this keeps the
model itself verified where there is no GPU."""
import numpy as np

from tests import prims_model as model


def _loop_sums(x):
    incl, excl, run = [], [], 0
    for v in x:
        excl.append(run)
        run += int(v)
        incl.append(run)
    return incl, excl


def _loop_seg_max(x, head):
    out, run = [], 0
    for v, h in zip(x, head):
        run = int(v) if h else max(run, int(v))
        out.append(run)
    return out


def _loop_sort(keys, vals, bits):
    """Insertion sort on (key mod 2^bits), strict comparison: an element never passes an equal one."""
    m = (1 << bits) - 1
    rows = []
    for k, v in zip(keys, vals):
        i = len(rows)
        while i > 0 and (rows[i - 1][0] & m) > (int(k) & m):
            i -= 1
        rows.insert(i, (int(k), int(v)))
    return [r[0] for r in rows], [r[1] for r in rows]


def _values(rng, n, kind):
    if kind == 0:
        return rng.integers(0, 4, n, dtype=np.uint32)
    if kind == 1:
        return rng.integers(0, 2 ** 32, n, dtype=np.uint32)
    return rng.choice(np.array([0, 1, 0xFFFFFFFE, 0xFFFFFFFF], dtype=np.uint32), n)


def test_sums_match_a_loop():
    rng = np.random.default_rng(101)
    for case in range(300):
        n = int(rng.integers(0, 201))
        x = _values(rng, n, case % 3)
        incl, excl = _loop_sums(x)
        assert model.inclusive_sum_u32(x).tolist() == [v % 2 ** 32 for v in incl]
        assert model.exclusive_sum_u32(x).tolist() == [v % 2 ** 32 for v in excl]
        got = model.exclusive_sum_u64(x)
        assert got.dtype == np.uint64 and got.tolist() == excl
    x = np.full(3, 0xFFFFFFFF, np.uint32)
    assert model.inclusive_sum_u32(x).tolist() == [0xFFFFFFFF, 0xFFFFFFFE, 0xFFFFFFFD]
    assert model.exclusive_sum_u64(x).tolist() == [0, 0xFFFFFFFF, 0x1FFFFFFFE]


def test_segmented_max_matches_a_loop():
    rng = np.random.default_rng(102)
    for case in range(300):
        n = int(rng.integers(0, 201))
        x = _values(rng, n, case % 3)
        density = (0.0, 0.05, 0.3, 1.0)[case % 4]
        head = np.where(rng.random(n) < density, rng.choice(np.array([1, 2, 0x80, 0xFF], dtype=np.uint8), n), 0).astype(np.uint8)
        assert model.segmented_inclusive_max_u32(x, head).tolist() == _loop_seg_max(x, head)
    # in front of the first head the maximum runs from 0; a head cuts a larger maximum off, 0xFFFFFFFF included
    x = np.array([5, 3, 0xFFFFFFFF, 0, 7, 2], np.uint32)
    head = np.array([0, 0, 0, 0x80, 0, 2], np.uint8)
    assert model.segmented_inclusive_max_u32(x, head).tolist() == [5, 5, 0xFFFFFFFF, 0, 7, 2]


def test_sort_matches_a_loop():
    rng = np.random.default_rng(103)
    for case in range(300):
        n = int(rng.integers(0, 201))
        wide = case % 2 == 1
        width = 64 if wide else 32
        bits = int(rng.integers(0, width + 1))
        keys = rng.integers(0, 2 ** width, n, dtype=np.uint64, endpoint=False).astype(np.uint64 if wide else np.uint32)
        if case % 3 == 0 and bits:   # few distinct sorted fields under random upper bits: ties everywhere
            low = rng.integers(0, min(1 << bits, 5), n, dtype=np.uint64)
            keys = ((keys.astype(np.uint64) & ~model.bit_mask(bits)) | low).astype(keys.dtype)
        vals = np.arange(n, dtype=np.uint32)
        k, v = model.radix_sort(keys, vals, bits)
        wk, wv = _loop_sort(keys, vals, bits)
        assert k.dtype == keys.dtype and k.tolist() == wk and v.tolist() == wv, (n, bits)
        k2, v2 = model.radix_sort(keys, None, bits)
        assert v2 is None and k2.tolist() == wk
        assert model.passes_in_second(bits) == len(range(0, bits, 8)) % 2


def test_sort_worked_example_bits_4():
    """Keys 0x10, 0x01 under bits = 4 have the fields 0 and 1: they stay as they are, whole; under bits = 8 they swap."""
    keys = np.array([0x10, 0x01], np.uint32)
    vals = np.array([0, 1], np.uint32)
    k, v = model.radix_sort(keys, vals, 4)
    assert k.tolist() == [0x10, 0x01] and v.tolist() == [0, 1]
    k, v = model.radix_sort(keys, vals, 8)
    assert k.tolist() == [0x01, 0x10] and v.tolist() == [1, 0]
    k, v = model.radix_sort(keys.astype(np.uint64), vals, 0)
    assert k.tolist() == [0x10, 0x01] and v.tolist() == [0, 1] and model.passes_in_second(0) == 0
