"""GPU route table (-m gpu) of the cascade's host driver (capi.hip: cascade_run_impl): which kernel serves which pass, for the
defaults and for every routing option one step away from its default, on five batches of one world.  Per pass the launch
report of mrg_cascade_stats (lds_mode, lds_bytes, group, n_launches, kbits_log2, pair_anchor, variant without bit 16, which
depends on the grid and so on the CU count: tests/test_gpu_dict.py covers it) and the processed / aligned counters, plus a
SHA-256 of the outputs, must equal tests/golden/cascade_routes.json exactly.  The fixture was recorded on the GPU by
tests/golden/make_cascade_routes_golden.py before the driver was restructured; the times and the search-internal counters
are not compared."""
import hashlib
import json
import os

import numpy as np
import pytest

from tests.util import LIB_ORDER, World

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cascade_routes.json")
FIELDS = ("lds_mode", "lds_bytes", "group", "n_launches", "kbits_log2", "pair_anchor", "variant", "processed", "aligned")
BATCHES = ("20..32", "16..19", "split", "long", "empty")
# the context's defaults of the options the cases move (capi.hip: struct mrg_ctx)
DEFAULTS = dict(fuse=1, seed_units=1, dict=1, split_mixed=1, pair_seeds=1, split_strata=1, pair_impl=1, stratum_rows=0,
                stratum0_unit=0, seed_impl=-1, seed_buckets=1, pos_scan=1, pair_big=5, round_large=0, kmer_filter=1,
                force_lds_mode=-1, lds_budget=160 * 1024, grid_pct=100, long_lane=0)
# (name, options away from their defaults, packed output form, batches)
CASES = [("defaults", {}, False, BATCHES), ("packed", {}, True, BATCHES)]
for _key, _values in (("fuse", (0, 2, 3)), ("seed_units", (0,)), ("dict", (0,)), ("split_mixed", (0,)), ("pair_seeds", (0,)),
                      ("pair_impl", (0,)), ("stratum_rows", (1, 2)), ("stratum0_unit", (1,)), ("seed_impl", (0, 1, 2)),
                      ("seed_buckets", (0,)), ("pos_scan", (0,)), ("pair_big", (0,)), ("round_large", (1,)), ("kmer_filter", (0,)),
                      ("force_lds_mode", (0, 1, 2, 3)), ("lds_budget", (49152,)), ("grid_pct", (50,))):
    for _v in _values:
        CASES.append(("%s=%d" % (_key, _v), {_key: _v}, False, BATCHES))
CASES.insert(7, ("pair_seeds=0,split_strata=0", dict(pair_seeds=0, split_strata=0), False, BATCHES))
CASES.append(("long_lane=1", dict(long_lane=1), False, ("split", "long")))


def make_world():
    """The world of tests/test_gpu_split.py: the small libraries, a 6.8 Mbp mRNA library, reads of 16..60 nt, reads with N."""
    return World(scale=0.05, n_fixed=12000, n_var=5000, with_n=True, max_var_len=60)


def make_engine(world):
    from mirge_amd.engine import Engine
    eng = Engine(0)
    for k in LIB_ORDER:
        eng.add_library(k, world.index[k])
    return eng


def make_batches(world, engine):
    """name -> ReadSet: the one-word N-free reads of 20..32 and of 16..19 nt, the whole two-word batch with its N mask (split),
    the reads over 32 nt only, and what Engine.prepare runs: zero one-word reads under the hints 16 / 32."""
    import torch
    from mirge_amd.engine import ReadSet
    clean = world.nmask[0] == 0
    out = {}
    for name, mask in (("20..32", (world.lens >= 20) & (world.lens <= 32) & clean), ("16..19", (world.lens >= 16) & (world.lens <= 19) & clean)):
        sel = np.flatnonzero(mask)
        assert len(sel) > 50, name
        out[name] = ReadSet(np.ascontiguousarray(world.words[:1, sel]), np.ascontiguousarray(world.lens[sel]), None, None, device=engine.device)
    out["split"] = ReadSet(world.words, world.lens, world.nmask, None, device=engine.device)
    sel = np.flatnonzero(world.lens > 32)
    assert len(sel) > 300
    out["long"] = ReadSet(np.ascontiguousarray(world.words[:, sel]), np.ascontiguousarray(world.lens[sel]),
                          np.ascontiguousarray(world.nmask[:, sel]), None, device=engine.device)
    out["empty"] = ReadSet.from_device(torch.empty((1, 0), dtype=torch.int64, device=engine.device),
                                       torch.empty(0, dtype=torch.uint8, device=engine.device), None, None, 16, 32)
    return out


def run_case(engine, batches, passes, options, packed, names):
    """One case on its batches -> {batch: {"passes": [[FIELDS...] per pass], "sha256": of the outputs}}; the options are
    back at their defaults afterwards."""
    out = {}
    for key, value in options.items():
        engine.set_option(key, value)
    try:
        for name in names:
            res = (engine.cascade_packed if packed else engine.cascade)(batches[name], passes)
            stats = res.stats
            h = hashlib.sha256()
            for a in ((res.packed.cpu().numpy(),) if packed else res.to_host()):
                h.update(np.ascontiguousarray(a).tobytes())
            rows = [[int(st[f]) & ~16 if f == "variant" else int(st[f]) for f in FIELDS] for st in stats]
            out[name] = dict(passes=rows, sha256=h.hexdigest())
    finally:
        for key in options:
            engine.set_option(key, DEFAULTS[key])
    return out


@pytest.fixture(scope="module")
def setup(native_lib):
    world = make_world()
    engine = make_engine(world)
    yield engine, make_batches(world, engine), engine.mirge_passes()
    engine.close()


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as fh:
        g = json.load(fh)
    assert tuple(g["fields"]) == FIELDS and sorted(g["cases"]) == sorted(c[0] for c in CASES)
    return g["cases"]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_cascade_routes_equal_the_recorded_table(setup, golden, case):
    engine, batches, passes = setup
    name, options, packed, names = case
    got = run_case(engine, batches, passes, options, packed, names)
    want = golden[name]
    assert sorted(got) == sorted(want), name
    for b in names:
        for i, (g, w) in enumerate(zip(got[b]["passes"], want[b]["passes"])):
            assert g == w, "%s, batch %s, pass %d: %s" % (name, b, i, dict(zip(FIELDS, zip(g, w))))
        assert len(got[b]["passes"]) == len(want[b]["passes"]), (name, b)
        assert got[b]["sha256"] == want[b]["sha256"], "%s, batch %s: the outputs differ" % (name, b)
