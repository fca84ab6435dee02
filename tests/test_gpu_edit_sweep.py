"""GPU parity (-m gpu) of the aligners over the edit sweep (tests/edit_sweep.py): every read length 16..32, every
single mismatch position at every site class (entry start / end, library start / end, offsets around the six- and
eight-bit segment-room fields, next to an N run), every pair of positions, triples for the 2-mismatch policy --
through every route to exact_dict_kernel, seed_kernel, wave_seed_kernel, pair_wave_kernel (csrc/dict.hip) and
match_kernel, fused_kernel, stratum_kernel (csrc/kernels.hip).  The yardstick is the exhaustive scan, computed once
per (library, policy); each route asserts from the pass statistics that the kernel it names ran, then for every read
that (entry, offset, mismatches) is the scan's, and the pass's processed / aligned counters are the scan's totals.
A failure names the route, the policy and the failing column of the grid (edit_sweep.grid_report).

Wall time of the module on an MI355X host with 16 CPUs: 24..27 s, nearly all of it the scans (xlarge 13.5 s for its
two policies, large 7.5 s for its four, small and small_n under half a second in all); the 87 cascades themselves
take under a second together."""
import numpy as np
import pytest

from tests import edit_sweep as es

pytestmark = pytest.mark.gpu

DECOY = dict(lib="decoy", seed_len=28, max_mm_seed=0, max_mm_total=2)   # launched first, claims nothing


class Rig:
    """One engine with the libraries of a sweep family, the decoy library, and the packed reads of each sweep."""

    def __init__(self, sweeps, exact_dict=None):
        from mirge_amd import pack
        from mirge_amd.engine import Engine, ReadSet
        from mirge_amd.index import FmIndex
        self.eng = Engine(0)
        self.eng.set_option("split_min_len", 0)     # the 16..19-nt reads too go to the dictionary kernels
        self.sweeps, self.reads = {}, {}
        for sw in sweeps:
            ix = FmIndex.build(sw.names, sw.seqs)
            self.eng.add_library(sw.name, ix, exact_dict=exact_dict)
            w, l, nm = pack.pack_reads([c.read for c in sw.cases])
            assert w.shape[0] == 1 and nm is None
            self.sweeps[sw.name] = sw
            self.reads[sw.name] = ReadSet(w, l, None, None, device=self.eng.device)
        self.eng.add_library("decoy", FmIndex.build(["decoy"], ["GATTACAGATTACAGGCCTTAAGGCCTTAACGCGCGTATATA" * 3]))

    def run(self, name, plan, **opts):
        """The cascade `plan` over the reads of sweep `name` under the options `opts` (restored afterwards):
        (host arrays, per-pass statistics)."""
        for k, v in opts.items():
            self.eng.set_option(k, v[0])
        try:
            res = self.eng.cascade(self.reads[name], self.eng.make_passes(plan))
            return res.to_host(), res.stats
        finally:
            for k, v in opts.items():
                self.eng.set_option(k, v[1])

    def close(self):
        self.eng.close()


@pytest.fixture(scope="module")
def small(native_lib, oracle_lib):
    rig = Rig(es.small_sweeps())
    yield rig
    rig.close()


@pytest.fixture(scope="module")
def large(native_lib, oracle_lib):
    rig = Rig([es.large_sweep()], exact_dict=True)
    yield rig
    rig.close()


@pytest.fixture(scope="module")
def xlarge(native_lib, oracle_lib):
    rig = Rig([es.xlarge_sweep()])
    yield rig
    rig.close()


def check(route, rig, name, policy, host, stats, k):
    """Pass k of the run against the scan: every read's (entry, offset, mismatches), unclaimed where the scan found
    nothing, processed / aligned; a decoy pass in front claimed nothing."""
    sw = rig.sweeps[name]
    scan = es.scan_answers(sw, policy)
    got = es.claimed(*host, k)
    report = es.grid_report("%s on %s" % (route, name), policy, sw.cases, got, scan)
    assert not report, report
    assert set(np.unique(host[0]).tolist()) <= {k, -1}, (route, name, policy)
    for i in range(k):
        assert (stats[i]["processed"], stats[i]["aligned"]) == (len(sw.cases), 0), (route, name, policy, i)
    assert (stats[k]["processed"], stats[k]["aligned"]) == (len(sw.cases), int((scan[:, 0] >= 0).sum())), (route, name, policy)
    print("%s on %s, policy %s: %d reads compared, %d aligned; lds_mode %d, variant %d, pair_anchor %d, launches %d" %
          (route, name, policy, len(sw.cases), stats[k]["aligned"], stats[k]["lds_mode"], stats[k]["variant"], stats[k]["pair_anchor"],
           stats[k]["n_launches"]))


def plan_of(policy, lib, decoy=False, tail=False):
    """The policy on `lib`; behind the decoy pass; with a `-v 0` pass on the same library behind it (what it could claim,
    every policy of the sweep has claimed: it only gives a fused launch its second member)."""
    return ([DECOY] if decoy else []) + [es.pass_dict(policy, lib)] + ([es.pass_dict(es.EXACT_POLICIES[1], lib)] if tail else [])


SMALL = ("small", "small_n")


@pytest.mark.parametrize("name", SMALL)
def test_route_1_exact_policies_alone_in_exact_dict_kernel(small, name):
    for policy in es.EXACT_POLICIES:
        host, st = small.run(name, plan_of(policy, name))
        assert st[0]["lds_mode"] == 7, st[0]
        check("route 1 (exact_dict_kernel)", small, name, policy, host, st, 0)


@pytest.mark.parametrize("name", SMALL)
def test_route_2_seed_kernel_units_behind_a_decoy(small, name):
    for policy in es.POLICIES[:4]:
        host, st = small.run(name, plan_of(policy, name, decoy=True))
        assert st[0]["lds_mode"] == 7 and st[1]["lds_mode"] in (8, 9) and st[1]["variant"] & 3 == 0 and st[1]["group"] == 1, st[:2]
        check("route 2 (seed_kernel unit)", small, name, policy, host, st, 1)


@pytest.mark.parametrize("name", SMALL)
def test_route_3_two_mismatches_in_pair_wave_kernel(small, name):
    host, st = small.run(name, plan_of(es.TWO_MM_POLICY, name, decoy=True))
    assert st[1]["lds_mode"] == 11 and st[1]["pair_anchor"] == 4, st[1]
    check("route 3 (pair_wave_kernel)", small, name, es.TWO_MM_POLICY, host, st, 1)
    host, st = small.run(name, plan_of(es.TWO_MM_POLICY, name))      # ... and reading the identity list
    assert st[0]["lds_mode"] == 11 and st[0]["pair_anchor"] == 4, st[0]
    check("route 3 (pair_wave_kernel, first launch)", small, name, es.TWO_MM_POLICY, host, st, 0)


@pytest.mark.parametrize("name", SMALL)
def test_route_4_two_mismatches_through_the_pigeonhole_pieces(small, name):
    """`pair_seeds` = 0: strata 1-2 and stratum 3 in match_kernel; `stratum_rows` = 2: both in stratum_kernel."""
    host, st = small.run(name, plan_of(es.TWO_MM_POLICY, name), pair_seeds=(0, 1))
    assert st[0]["lds_mode"] in (0, 1, 2, 3) and st[0]["pair_anchor"] == 0 and st[0]["n_launches"] == 2, st[0]
    check("route 4 (match_kernel, strata)", small, name, es.TWO_MM_POLICY, host, st, 0)
    host, st = small.run(name, plan_of(es.TWO_MM_POLICY, name), pair_seeds=(0, 1), stratum_rows=(2, 0))
    assert st[0]["lds_mode"] in (5, 6) and st[0]["pair_anchor"] == 0 and st[0]["n_launches"] == 2, st[0]
    check("route 4 (stratum_kernel, pieces)", small, name, es.TWO_MM_POLICY, host, st, 0)


@pytest.mark.parametrize("name", SMALL)
def test_route_5_the_fm_kernels(small, name):
    """`dict` = 0.  A pass alone runs match_kernel (the 2-mismatch policy: stratum_kernel over the anchor pairs); `fuse`
    changes the kernel only where two passes of at most one seed mismatch follow a first launch: the policy between
    the decoy pass and a `-v 0` pass on its own library runs in fused_kernel."""
    for policy in es.POLICIES:
        host, st = small.run(name, plan_of(policy, name), dict=(0, 1))
        if policy[1] == 2:
            assert st[0]["lds_mode"] in (5, 6) and st[0]["pair_anchor"] == 4, st[0]
        else:
            assert st[0]["lds_mode"] in (0, 1, 2, 3), st[0]
        check("route 5 (FM kernels, alone)", small, name, policy, host, st, 0)
    for policy in es.POLICIES[:4]:
        host, st = small.run(name, plan_of(policy, name, decoy=True, tail=True), dict=(0, 1))
        assert st[1]["lds_mode"] == 4 and st[2]["lds_mode"] == 4 and st[2]["group"] == 1, st
        check("route 5 (fused_kernel)", small, name, policy, host, st, 1)
        host, st = small.run(name, plan_of(policy, name, decoy=True, tail=True), dict=(0, 1), fuse=(0, 1))
        assert st[1]["lds_mode"] in (0, 1, 2, 3) and st[1]["group"] == 1 and st[2]["group"] == 2, st
        check("route 5 (match_kernel behind a list)", small, name, policy, host, st, 1)


def test_route_6_one_mismatch_on_the_large_library(large):
    """A seed launch searches a library of at most 2^22 bases through an index rebuilt from its entries: no seed buckets
    (`lds_mode` 8) and hence no anchor pairs (`pair_anchor` 0 whatever `pair_big` says: only wave_seed_kernel's
    instantiation with buckets takes them), in seed_kernel by default and in wave_seed_kernel with `seed_impl` = 2.
    The library's own device-built tables equal the host's word for word."""
    assert large.eng.check_tables("large") == dict(jump_tables=0, row_context=0, wide_rows=0, seed_buckets=0)
    for policy in es.ONE_MM_POLICIES:
        for seed_impl, variant in ((2, 2), (-1, 0)):
            for seed_buckets in (1, 0):
                for pair_big in (5, 0):
                    host, st = large.run("large", plan_of(policy, "large", decoy=True), seed_buckets=(seed_buckets, 1), pair_big=(pair_big, 5),
                                         seed_impl=(seed_impl, -1))
                    route = "route 6 (%s, seed_buckets %d, pair_big %d)" % ("wave_seed_kernel" if variant else "seed_kernel", seed_buckets, pair_big)
                    assert st[1]["lds_mode"] == 8 and st[1]["variant"] & 3 == variant and st[1]["group"] == 1, (route, st[1])
                    assert st[1]["pair_anchor"] == 0, (route, st[1])
                    check(route, large, "large", policy, host, st, 1)


def test_route_6_wave_seed_kernel_with_seed_buckets(xlarge):
    """Past 2^22 bases a seed launch searches the library's own arrays in wave_seed_kernel (the default there): seed
    buckets (`lds_mode` 9) and position lists or, `seed_buckets` = 0, the jump tables (8); with buckets and `pair_big`
    = 5 the 16..19-nt reads go through the device-built tables of three 5-base anchor pairs (`pair_anchor` 5), otherwise
    through the pigeonhole pieces: the same answers."""
    assert xlarge.eng.check_tables("xlarge") == dict(jump_tables=0, row_context=0, wide_rows=0, seed_buckets=0)
    for policy in es.XLARGE_POLICIES:
        for seed_buckets in (1, 0):
            for pair_big in (5, 0):
                host, st = xlarge.run("xlarge", plan_of(policy, "xlarge", decoy=True), seed_buckets=(seed_buckets, 1), pair_big=(pair_big, 5))
                route = "route 6 (wave_seed_kernel past 2^22 bases, seed_buckets %d, pair_big %d)" % (seed_buckets, pair_big)
                assert st[1]["lds_mode"] == (9 if seed_buckets else 8) and st[1]["variant"] & 3 == 2 and st[1]["group"] == 1, (route, st[1])
                assert st[1]["pair_anchor"] == (pair_big if seed_buckets else 0), (route, st[1])
                check(route, xlarge, "xlarge", policy, host, st, 1)


def test_route_7_exact_policies_alone_on_the_large_library(large):
    for policy in es.EXACT_POLICIES:
        host, st = large.run("large", plan_of(policy, "large"))
        assert st[0]["lds_mode"] == 7, st[0]
        check("route 7 (exact_dict_kernel)", large, "large", policy, host, st, 0)


def test_route_8_exact_policies_as_a_dictionary_unit(large):
    for policy in es.EXACT_POLICIES:
        for seed_impl, variant in ((-1, 0), (2, 2)):     # the unit in seed_kernel / in wave_seed_kernel
            host, st = large.run("large", plan_of(policy, "large", decoy=True), seed_impl=(seed_impl, -1))
            assert st[1]["lds_mode"] in (8, 9) and st[1]["variant"] & 3 == variant and st[1]["group"] == 1, st[1]
            check("route 8 (dictionary unit of a seed launch, seed_impl %d)" % seed_impl, large, "large", policy, host, st, 1)


def test_route_9_the_fm_kernels_on_the_large_library(large):
    for policy in es.LARGE_POLICIES:
        host, st = large.run("large", plan_of(policy, "large"), dict=(0, 1))
        assert st[0]["lds_mode"] in (0, 1, 2, 3), st[0]
        check("route 9 (match_kernel)", large, "large", policy, host, st, 0)
    for policy in es.ONE_MM_POLICIES:      # fused_kernel with the three anchor pairs for the 16..19-nt reads
        host, st = large.run("large", plan_of(policy, "large", decoy=True, tail=True), dict=(0, 1))
        assert st[1]["lds_mode"] == 4 and st[1]["pair_anchor"] == 5, st[1]
        check("route 9 (fused_kernel, pair_big 5)", large, "large", policy, host, st, 1)
