"""The scratch sizes the library reports, without a GPU: every mrg_*_temp_bytes call of the stages that carve a caller's
scratch (capi.hip: Carver and the layout structs on top of it) returns, byte for byte, what tests/golden/scratch_bytes.json
holds.  The fixture was recorded (tests/golden/make_scratch_bytes_golden.py) from the library as it was before the layouts
were rewritten on the one carver, so a layout that gains, loses or re-rounds a piece shows here.

The sizes are those at which a rounding changes the result: around the 8- and 256-byte steps, odd and even counts (the
trim stage keeps its uint64 array aligned with an even count of uint32), the primitives' tile boundaries, and each call's
documented limit."""
import ctypes as C
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scratch_bytes.json")

SIZES = (0, 1, 2, 3, 7, 8, 9, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 65535, 65536, 65537, 2 ** 20, 2 ** 24 + 1)
# call -> the documented limit of each size argument (include/mirge_amd.h)
LIMITS = {
    "mrg_predict_trim_temp_bytes": (2 ** 31 - 1,),
    "mrg_predict_remap_temp_bytes": (2 ** 31 - 1, 2 ** 32 - 2),
    "mrg_predict_feature_temp_bytes": (2 ** 32 - 2,),
    "mrg_predict_precursor_temp_bytes": (2 ** 30 - 1,),
    "mrg_predict_screen_temp_bytes": (2 ** 30 - 4,),
    "mrg_predict_reads_temp_bytes": (2 ** 31 - 1,),
    "mrg_collapsed_order_temp_bytes": (2 ** 31 - 1,),
}
N_OUT = {"mrg_collapsed_order_temp_bytes": 2}


def arguments(call):
    """The size tuples a call is recorded at: every size and the limit; the two-argument call over the whole grid."""
    axes = [SIZES + (lim,) for lim in LIMITS[call]]
    if len(axes) == 1:
        return [(n,) for n in axes[0]]
    return [(a, b) for a in axes[0] for b in axes[1]]


def record(lib):
    """{call: [[*sizes, *bytes], ...]} from the loaded library; a call that fails is an error here, not a value."""
    out = {}
    for call in LIMITS:
        rows = []
        for sizes in arguments(call):
            res = [C.c_uint64() for _ in range(N_OUT.get(call, 1))]
            rc = getattr(lib, call)(*sizes, *[C.byref(r) for r in res])
            assert rc == 0, "%s%r: %s" % (call, sizes, lib.mrg_last_error())
            rows.append(list(sizes) + [r.value for r in res])
        out[call] = rows
    return out


@pytest.mark.parametrize("call", sorted(LIMITS))
def test_sizes_equal_the_recorded_ones(native_lib, call):
    with open(GOLDEN) as fh:
        want = json.load(fh)["calls"]
    got = record(native_lib)[call]
    assert len(got) == len(want[call]) == len(arguments(call))
    assert got == want[call]


def test_one_past_each_limit_is_refused(native_lib):
    for call, limits in LIMITS.items():
        for i, lim in enumerate(limits):
            sizes = [0] * len(limits)
            sizes[i] = lim + 1
            res = [C.c_uint64() for _ in range(N_OUT.get(call, 1))]
            assert getattr(native_lib, call)(*sizes, *[C.byref(r) for r in res]) < 0, (call, sizes)
            assert b"limit" in native_lib.mrg_last_error()
