"""GPU (-m gpu): the device primitives of csrc/prims.hip called directly (mrg_prims_*) -- the three prefix sums, the
segmented inclusive max-scan and the stable radix sort -- against the numpy model (tests/prims_model.py, itself pinned
by tests/test_prims_model.py), for exact equality: these are integer operations, there is no tolerance anywhere.

Every output buffer carries 64 guard elements behind index n - 1 and the scratch a 256-byte guard behind the size
mrg_prims_temp_bytes reports; the scratch is handed over full of a non-zero pattern.  Every guard must come back
untouched: that is the check of the hand-derived scan_temp_bytes / radix_temp_bytes.

Sizes cross the thread (16), wave (1024) and tile (4096) boundaries and, for the scans, the third level: above
4096^2 = 16 777 216 elements scan_impl / seg_max_impl recurse twice.  The sort's own count scan reaches its third level
only above 2^24 counts = 65 536 tiles, i.e. more than 2.6 * 10^8 keys (2 GiB of 64-bit keys in each of two buffers):
out of reach of a test of seconds and NOT tested here; the three-level scan tests run that code (the same scan_impl)."""
import ctypes as C

import numpy as np
import pytest

from tests import prims_model as model

pytestmark = pytest.mark.gpu

GUARD = 64            # elements behind every output
TMP_GUARD = 256       # bytes behind the scratch
PAT = 0xA5            # every guard byte

SCAN, SORT = 0, 1                                   # mrg_prims_temp_bytes kinds
EXCL_U32, INCL_U32, EXCL_U64 = 0, 1, 2              # mrg_prims_scan kinds

TILE = 4096
SMALL = [0, 1, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 8193]
BIG = [TILE * TILE - 1, TILE * TILE, TILE * TILE + 1, TILE * TILE + 4097]      # two recursions above 4096^2
HEAD_BYTES = np.array([1, 2, 0x80, 0xFF], dtype=np.uint8)


class Prims:
    def __init__(self):
        import torch
        from mirge_amd.engine import Engine
        self.torch = torch
        self.eng = Engine(0)
        self.lib = self.eng._lib
        self.dev = self.eng.device

    # -- buffers: bytes on the device, `guard` pattern elements behind the payload
    def up(self, arr, guard=GUARD):
        arr = np.ascontiguousarray(arr)
        buf = np.empty(arr.size + guard, arr.dtype)
        buf[:arr.size] = arr
        buf[arr.size:].view(np.uint8)[:] = PAT
        return self.torch.from_numpy(buf.view(np.uint8)).to(self.dev)

    def blank(self, n, dtype, guard=GUARD):
        return self.torch.full(((n + guard) * np.dtype(dtype).itemsize,), PAT, dtype=self.torch.uint8, device=self.dev)

    def down(self, t, n, dtype, what):
        """The payload of a buffer; its guard must be untouched."""
        a = t.cpu().numpy().view(dtype)
        assert (a[n:].view(np.uint8) == PAT).all(), "%s: written behind index n - 1" % what
        return a[:n]

    def scratch(self, kind, n):
        need = C.c_uint64()
        assert self.lib.mrg_prims_temp_bytes(kind, n, C.byref(need)) == 0
        return self.blank(need.value, np.uint8, TMP_GUARD), need.value

    def check_scratch(self, tmp, need, what):
        assert bool((tmp[need:] == PAT).all()), "%s: written behind the %d scratch bytes" % (what, need)

    def sync(self):
        self.torch.cuda.current_stream(self.dev).synchronize()

    def ok(self, rc):
        assert rc == 0, self.lib.mrg_last_error()

    # -- the calls
    def scan(self, kind, x, inplace=False):
        n = x.size
        odt = np.uint64 if kind == EXCL_U64 else np.uint32
        d_in = self.up(x)
        d_out = d_in if inplace else self.blank(n, odt)
        tmp, need = self.scratch(SCAN, n)
        self.ok(self.lib.mrg_prims_scan(self.eng._h, kind, d_in.data_ptr(), d_out.data_ptr(), n, tmp.data_ptr(), need,
                                        self.eng._stream_ptr()))
        self.sync()
        what = "scan kind %d n %d%s" % (kind, n, " in place" if inplace else "")
        self.check_scratch(tmp, need, what)
        if not inplace:
            assert np.array_equal(self.down(d_in, n, np.uint32, what), x), what + ": the input changed"
        return self.down(d_out, n, odt, what)

    def segmax(self, x, head, inplace=False):
        n = x.size
        d_in, d_head = self.up(x), self.up(head)
        d_out = d_in if inplace else self.blank(n, np.uint32)
        tmp, need = self.scratch(SCAN, n)
        self.ok(self.lib.mrg_prims_segmented_max(self.eng._h, d_in.data_ptr(), d_head.data_ptr(), d_out.data_ptr(), n,
                                                 tmp.data_ptr(), need, self.eng._stream_ptr()))
        self.sync()
        what = "segmented max n %d%s" % (n, " in place" if inplace else "")
        self.check_scratch(tmp, need, what)
        assert np.array_equal(self.down(d_head, n, np.uint8, what), head), what + ": the heads changed"
        return self.down(d_out, n, np.uint32, what)

    def sort(self, keys, vals, bits):
        """-> (keys, vals or None, in_second) as the call left them in the buffer it names."""
        n, kdt = keys.size, keys.dtype
        k = [self.up(keys), self.blank(n, kdt)]
        v = [self.up(vals), self.blank(n, np.uint32)] if vals is not None else [None, None]
        tmp, need = self.scratch(SORT, n)
        second = C.c_int32(-1)
        self.ok(self.lib.mrg_prims_radix_sort(self.eng._h, kdt.itemsize, k[0].data_ptr(), k[1].data_ptr(),
                                              v[0].data_ptr() if vals is not None else None,
                                              v[1].data_ptr() if vals is not None else None, n, bits, tmp.data_ptr(), need,
                                              C.byref(second), self.eng._stream_ptr()))
        self.sync()
        what = "sort u%d n %d bits %d%s" % (8 * kdt.itemsize, n, bits, "" if vals is not None else " keys only")
        self.check_scratch(tmp, need, what)
        assert second.value in (0, 1), what
        got = [self.down(t, n, kdt, what) for t in k]
        gotv = [self.down(t, n, np.uint32, what) for t in v] if vals is not None else [None, None]
        if n == 0 or bits == 0:     # nothing moves: the input where it was, the second buffers untouched
            assert second.value == 0, what
            assert (got[1].view(np.uint8) == PAT).all(), what
            assert vals is None or (gotv[1].view(np.uint8) == PAT).all(), what
        return got[second.value], gotv[second.value], second.value


@pytest.fixture(scope="module")
def prims(native_lib):
    return Prims()


# ------------------------------------------------------------------------------------------------ prefix sums
def _sum_inputs(rng, n):
    """name -> uint32 input of n elements (the issue's list)."""
    out = {"ones": np.ones(n, np.uint32),
           "small": rng.integers(0, 4, n, dtype=np.uint32),
           "full": rng.integers(0, 2 ** 32, n, dtype=np.uint32)}
    for name, idx in (("first", [0]), ("last", [n - 1]), ("tile_ends", list(range(TILE - 1, n, TILE)))):
        x = np.zeros(n, np.uint32)
        if n:
            x[idx] = 0xFFFFFFF1
        out[name] = x
    return out


def _check_sums(prims, x, tag, inplace_too=True):
    want = {EXCL_U32: model.exclusive_sum_u32(x), INCL_U32: model.inclusive_sum_u32(x), EXCL_U64: model.exclusive_sum_u64(x)}
    for kind in (EXCL_U32, INCL_U32, EXCL_U64):
        for inplace in ((False, True) if inplace_too and kind != EXCL_U64 else (False,)):
            got = prims.scan(kind, x, inplace)
            bad = np.flatnonzero(got != want[kind])
            assert bad.size == 0, "%s kind %d inplace %s: first wrong index %d (got %d, want %d)" % (
                tag, kind, inplace, bad[0], got[bad[0]], want[kind][bad[0]])


@pytest.mark.parametrize("n", SMALL)
def test_sums_small_sizes(prims, n):
    """All three sums, in place and out of place for the 32-bit kinds, on every input pattern; n = 0 succeeds and
    leaves every buffer as it was."""
    rng = np.random.default_rng(1000 + n)
    for name, x in _sum_inputs(rng, n).items():
        _check_sums(prims, x, "n %d %s" % (n, name))


@pytest.mark.parametrize("n", BIG)
def test_sums_three_levels(prims, n):
    """Around 4096^2 elements, where the tile sums' scan itself has more than one tile of tile sums: once per sum (the
    exclusive one in place, the inclusive one out of place), on full-range values -- the 32-bit sums wrap at once and
    the 64-bit sums pass 2^32 within the first elements, so a wrong or missing offset at any level shows in every
    element behind it."""
    x = np.random.default_rng(n).integers(0, 2 ** 32, n, dtype=np.uint32)
    excl = model.exclusive_sum_u64(x)
    got = prims.scan(EXCL_U64, x)
    assert np.array_equal(got, excl), "u64 n %d: first wrong index %d" % (n, np.flatnonzero(got != excl)[0])
    want = excl.astype(np.uint32)
    got = prims.scan(EXCL_U32, x, inplace=True)
    assert np.array_equal(got, want), "exclusive n %d: first wrong index %d" % (n, np.flatnonzero(got != want)[0])
    want += x
    got = prims.scan(INCL_U32, x)
    assert np.array_equal(got, want), "inclusive n %d: first wrong index %d" % (n, np.flatnonzero(got != want)[0])


def test_sums_three_levels_tile_ends(prims):
    """One non-zero at every tile's last element and at the very end, 4096^2 + 4097 elements: every tile sum and every
    second-level tile sum is the carry of exactly one element."""
    n = BIG[-1]
    x = np.zeros(n, np.uint32)
    x[TILE - 1::TILE] = 1
    x[-1] = 7
    want = model.inclusive_sum_u32(x)
    got = prims.scan(INCL_U32, x, inplace=True)
    assert np.array_equal(got, want), "first wrong index %d" % np.flatnonzero(got != want)[0]


# ------------------------------------------------------------------------------------------------ segmented max-scan
def _head_patterns(rng, n):
    """name -> uint8 heads of n elements (the issue's list); the head bytes come from {1, 2, 0x80, 0xFF}."""
    byte = rng.choice(HEAD_BYTES, n)
    i = np.arange(n)
    out = {"none": np.zeros(n, np.uint8), "every": byte.copy()}
    for name, idx in (("first", 0), ("last", n - 1)):
        h = np.zeros(n, np.uint8)
        if n:
            h[idx] = byte[idx]
        out[name] = h
    for step in (16, 1024, 4096):
        for shift in (-1, 0, 1):
            out["every%d%+d" % (step, shift)] = np.where((i - shift) % step == 0, byte, 0).astype(np.uint8)
    for name, p in (("third", 1 / 3), ("sparse", 1 / 5000)):
        out[name] = np.where(rng.random(n) < p, byte, 0).astype(np.uint8)
    return out


def _seg_values(rng, n):
    edge = rng.integers(0, 2 ** 32, n, dtype=np.uint32)
    pick = rng.random(n)
    edge[pick < 0.2] = 0
    edge[pick > 0.8] = 0xFFFFFFFF
    # falling: the maximum of a segment is at its head, so every later element needs the carry from there
    return {"small": rng.integers(0, 4, n, dtype=np.uint32),
            "full": rng.integers(0, 2 ** 32, n, dtype=np.uint32),
            "edge": edge,
            "falling": (np.uint32(0xFFFFFFFF) - np.arange(n, dtype=np.uint32))}


def _check_segmax(prims, x, head, tag, placements=(False, True)):
    want = model.segmented_inclusive_max_u32(x, head)
    for inplace in placements:
        got = prims.segmax(x, head, inplace)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, "%s inplace %s: first wrong index %d (got %#x, want %#x)" % (
            tag, inplace, bad[0], got[bad[0]], want[bad[0]])


@pytest.mark.parametrize("n", SMALL)
def test_segmented_max_small_sizes(prims, n):
    """Every value kind crossed with every head pattern, in place and out of place; n = 0 succeeds and leaves every
    buffer as it was."""
    rng = np.random.default_rng(2000 + n)
    values, heads = _seg_values(rng, n), _head_patterns(rng, n)
    for vname, x in values.items():
        for hname, head in heads.items():
            _check_segmax(prims, x, head, "n %d %s/%s" % (n, vname, hname))


@pytest.mark.parametrize("n", BIG)
def test_segmented_max_three_levels(prims, n):
    """Around 4096^2 elements, once per size: values that fall slowly (each segment's maximum is near its head, so the
    carry of every level decides most elements) with a little noise (so the local values decide some), heads at 1 in 5000
    in the first quarter and a dozen in the rest, elements in front of the first head.  In place for the even sizes."""
    rng = np.random.default_rng(n)
    x = np.uint32(0xFFFFFFF0) - np.arange(n, dtype=np.uint32) + rng.integers(0, 9, n, dtype=np.uint32)
    head = np.zeros(n, np.uint8)
    q = n // 4
    dense = np.flatnonzero(rng.random(q) < 1 / 5000)
    head[dense] = rng.choice(HEAD_BYTES, dense.size)
    head[rng.integers(q, n, 12)] = rng.choice(HEAD_BYTES, 12)
    head[:3] = 0
    _check_segmax(prims, x, head, "n %d" % n, placements=(n % 2 == 0,))


def test_segmented_max_planted_carry_through_every_level(prims):
    """4096^2 + 4097 elements: the maximum 0xFFFFFFFE sits in tile 0 in front of any head and there is no head until one
    element before the end, so it is carried through both upper levels into every tile -- and the head at n - 2 must cut
    it off."""
    n = BIG[-1]
    x = np.random.default_rng(7).integers(0, 1000, n, dtype=np.uint32)
    x[5] = 0xFFFFFFFE
    head = np.zeros(n, np.uint8)
    head[n - 2] = 0x80
    want = model.segmented_inclusive_max_u32(x, head)
    assert want[4] < 1000 and (want[5:n - 2] == 0xFFFFFFFE).all() and want[n - 2] == x[n - 2] and want[n - 1] == max(x[n - 2:])
    _check_segmax(prims, x, head, "planted", placements=(False,))


# ------------------------------------------------------------------------------------------------ radix sort
SORT_SIZES = [0, 1, 63, 64, 65, 4095, 4096, 4097, 65_536, 65_537, 1_100_003]
SORT_BITS = {4: [0, 1, 7, 8, 9, 17, 31, 32], 8: [0, 1, 8, 9, 33, 60, 63, 64]}
ODD_BITS = {4: 17, 8: 33}
PATTERNS = ("equal", "two", "rows", "sorted", "descending", "random")


def _sort_keys(rng, pattern, n, key_bytes, bits):
    """n keys whose SORTED FIELD (bits [0, bits)) follows `pattern` and whose bits above it are random garbage: the
    sort must order by the field alone, keep equal fields in input order and carry the garbage along."""
    width = 8 * key_bytes
    i = np.arange(n, dtype=np.uint64)
    top = (1 << bits)       # fields are below this
    if pattern == "equal":          # one digit owns whole tiles
        low = np.full(n, 0xA5A5A5A5A5A5A5A5 % top, np.uint64)
    elif pattern == "two":          # two values alternating by lane
        low = np.where(i % np.uint64(2) == 0, np.uint64(0x5A3C96E1D2B4F087 % top), np.uint64(0x0123456789ABCDEF % top))
    elif pattern == "rows":         # every row of 64 lanes holds all of 0..63 in every 8-bit digit
        d = (i * np.uint64(37) + i // np.uint64(64)) % np.uint64(64)
        low = np.zeros(n, np.uint64)
        for p in range(0, bits, 8):
            low |= d << np.uint64(p)
        low &= model.bit_mask(bits)
    elif pattern == "sorted":
        low = np.sort(rng.integers(0, top, n, dtype=np.uint64))
    elif pattern == "descending":   # strictly where the field has room for n values
        if top > n:
            low = (np.uint64(max(n, 1) - 1) - i) * np.uint64((top - 1) // max(n, 1))
        else:
            low = (np.uint64(n - 1) - i) * np.uint64(top) // np.uint64(n)
    else:
        low = rng.integers(0, top, n, dtype=np.uint64)
    garbage = rng.integers(0, 2 ** width, n, dtype=np.uint64) & ~model.bit_mask(bits)
    return (garbage | low).astype(np.uint64 if key_bytes == 8 else np.uint32)


def _check_sort(prims, keys, bits, with_vals, tag):
    n = keys.size
    vals = np.arange(n, dtype=np.uint32) if with_vals else None      # iota: stability is visible
    wk, wv = model.radix_sort(keys, vals, bits)
    gk, gv, second = prims.sort(keys, vals, bits)
    if n and bits:
        assert second == model.passes_in_second(bits), "%s: in_second %d after %d passes" % (tag, second, (bits + 7) // 8)
    bad = np.flatnonzero(gk != wk)
    assert bad.size == 0, "%s: keys first wrong at %d (got %#x, want %#x)" % (tag, bad[0], gk[bad[0]], wk[bad[0]])
    if with_vals:
        bad = np.flatnonzero(gv != wv)
        assert bad.size == 0, "%s: values first wrong at %d (got %d, want %d)" % (tag, bad[0], gv[bad[0]], wv[bad[0]])


@pytest.mark.parametrize("n", SORT_SIZES)
@pytest.mark.parametrize("key_bytes", [4, 8])
def test_sort_sizes(prims, key_bytes, n):
    """Every size at the full key width and at one odd width (17 / 33 bits, garbage above), pairs and keys only, every
    key pattern -- at 1 100 003 keys the patterns that depend on the size: random (pairs and keys only), two values and
    all equal (pairs)."""
    rng = np.random.default_rng(3000 + n + key_bytes)
    big = n > 100_000
    for bits in (8 * key_bytes, ODD_BITS[key_bytes]):
        for pattern in (("random", "two", "equal") if big else PATTERNS):
            keys = _sort_keys(rng, pattern, n, key_bytes, bits)
            for with_vals in ((True, False) if not big or pattern == "random" else (True,)):
                _check_sort(prims, keys, bits, with_vals, "u%d n %d bits %d %s vals %s" % (8 * key_bytes, n, bits, pattern, with_vals))


@pytest.mark.parametrize("n", [4097, 65_537])
@pytest.mark.parametrize("key_bytes,bits", [(kb, b) for kb in (4, 8) for b in SORT_BITS[kb]])
def test_sort_every_width(prims, key_bytes, bits, n):
    """Every `bits` value at a size just above one tile and at the size where the count scan goes to two levels:
    random garbage above `bits` pins "stable over key bits [0, bits)"; bits = 0 leaves the input where it was."""
    rng = np.random.default_rng(4000 + n + 100 * bits + key_bytes)
    for pattern in PATTERNS:
        keys = _sort_keys(rng, pattern, n, key_bytes, bits)
        for with_vals in (True, False):
            _check_sort(prims, keys, bits, with_vals, "u%d n %d bits %d %s vals %s" % (8 * key_bytes, n, bits, pattern, with_vals))


@pytest.mark.parametrize("key_bytes", [4, 8])
def test_sort_worked_example_bits_4(prims, key_bytes):
    """Keys 0x10, 0x01 under bits = 4 have the fields 0 and 1 and stay as they are."""
    keys = np.array([0x10, 0x01], np.uint64 if key_bytes == 8 else np.uint32)
    gk, gv, second = prims.sort(keys, np.array([0, 1], np.uint32), 4)
    assert gk.tolist() == [0x10, 0x01] and gv.tolist() == [0, 1] and second == 1


def test_bad_arguments_are_refused(prims):
    """With a live context: undersized scratch, oversize bits, unknown kinds, one value buffer without the other."""
    from mirge_amd._native import MRG_ERR_ARG
    L, h, st = prims.lib, prims.eng._h, prims.eng._stream_ptr()
    buf = prims.blank(10_000, np.uint64)
    p = buf.data_ptr()
    tmp, need = prims.scratch(SCAN, 10_000)
    assert need > 0
    assert L.mrg_prims_scan(h, INCL_U32, p, p, 10_000, tmp.data_ptr(), need - 1, st) == MRG_ERR_ARG
    assert L.mrg_prims_scan(h, 3, p, p, 10_000, tmp.data_ptr(), need, st) == MRG_ERR_ARG
    assert L.mrg_prims_scan(h, INCL_U32, None, p, 10_000, tmp.data_ptr(), need, st) == MRG_ERR_ARG
    assert L.mrg_prims_segmented_max(h, p, p, p, 10_000, tmp.data_ptr(), need - 1, st) == MRG_ERR_ARG
    assert L.mrg_prims_segmented_max(h, p, None, p, 10_000, tmp.data_ptr(), need, st) == MRG_ERR_ARG
    tmp, need = prims.scratch(SORT, 10_000)
    second = C.c_int32()
    assert L.mrg_prims_radix_sort(h, 8, p, p, None, None, 10_000, 64, tmp.data_ptr(), need - 1, C.byref(second), st) == MRG_ERR_ARG
    assert L.mrg_prims_radix_sort(h, 8, p, p, None, None, 10_000, 65, tmp.data_ptr(), need, C.byref(second), st) == MRG_ERR_ARG
    assert L.mrg_prims_radix_sort(h, 4, p, p, None, None, 10_000, 33, tmp.data_ptr(), need, C.byref(second), st) == MRG_ERR_ARG
    assert L.mrg_prims_radix_sort(h, 2, p, p, None, None, 10_000, 8, tmp.data_ptr(), need, C.byref(second), st) == MRG_ERR_ARG
    assert L.mrg_prims_radix_sort(h, 8, p, p, p, None, 10_000, 8, tmp.data_ptr(), need, C.byref(second), st) == MRG_ERR_ARG
    assert L.mrg_prims_radix_sort(h, 8, p, None, None, None, 10_000, 8, tmp.data_ptr(), need, C.byref(second), st) == MRG_ERR_ARG
    assert L.mrg_prims_radix_sort(h, 8, p, p, None, None, 10_000, 8, tmp.data_ptr(), need, None, st) == MRG_ERR_ARG
    assert L.mrg_prims_radix_sort(h, 8, p, p, None, None, 2 ** 32 - 1, 8, tmp.data_ptr(), need, C.byref(second), st) == MRG_ERR_ARG
    prims.sync()
    assert bool((buf == PAT).all()), "a refused call wrote"
