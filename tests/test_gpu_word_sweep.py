"""GPU parity (-m gpu) of the aligners over the word sweep (tests/word_sweep.py): reads of 33..255 nt on the edges of
every word count and reads with an N, in batches of W = 2, 4 and 8 words with an N mask -- a substitution and an N on
every base at every site class, pairs and triples around every word boundary, T tails that begin on either side of
one -- through every route to match_kernel<W>, fused_kernel<W>, stratum_kernel<W> (csrc/kernels.hip), through the
split of a mixed batch, and through the LONG instantiations of seed_kernel, wave_seed_kernel and pair_wave_kernel
(csrc/dict.hip).  As in tests/test_gpu_edit_sweep.py the yardstick is the exhaustive scan, computed once per (batch,
policy); each route asserts from the pass statistics that the kernel it names ran, then that every read's (entry,
offset, mismatches) is the scan's and the pass's processed / aligned counters are the scan's totals.  A failure names
the route, the policy and the failing (L, edit position) of the grid (edit_sweep.grid_report).

Wall time: the scans of the module (15 of the grid, 15 of the poly-T classes) take 10.5 s on a host with 8 CPUs and no
GPU (w8 4.6 s, w4 2.7 s, w2 3.0 s, the poly-T classes 0.2 s).  The whole module on an MI355X host with 16 CPUs: 5.4 s
(2.1 s building the rig, 2.4 s the scans, the 133 cascades a tenth of a second together) -- against the 24..27 s of
the edit sweep's module, the yardstick.  Nothing of the grid was thinned: B(L) x B(L) is swept in full.
"""
import numpy as np
import pytest

from tests import edit_sweep as es
from tests import word_sweep as ws

pytestmark = pytest.mark.gpu

DECOY = dict(lib="decoy", seed_len=28, max_mm_seed=0, max_mm_total=2)   # launched first, claims nothing
WORDS = (2, 4, 8)
MATCH, STRATUM, FUSED, EXACT, SEED, PAIR_WAVE = (0, 1, 2, 3), (5, 6), (4,), (7,), (8, 9), (11,)   # mrg_pass_stats.lds_mode
LONG = 8                                                                                             # mrg_pass_stats.variant


class Rig:
    """One engine with the sweep's library and the decoy library, and one ReadSet per batch with its N mask."""

    def __init__(self):
        from mirge_amd.engine import Engine, ReadSet
        from mirge_amd.index import FmIndex
        self.eng = Engine(0)
        self.sweeps = ws.word_sweeps()
        lib = self.sweeps["w2"]
        self.eng.add_library("lib", FmIndex.build(lib.names, lib.seqs))
        self.eng.add_library("decoy", FmIndex.build(["decoy"], ["GATTACAGATTACAGGCCTTAAGGCCTTAACGCGCGTATATA" * 3]))
        self.reads = {}
        for name, sw in self.sweeps.items():
            w, l, nm = ws.pack(sw)
            assert w.shape[0] == int(name[1]) and nm is not None
            self.reads[name] = ReadSet(w, l, nm, None, device=self.eng.device)

    def run(self, name, plan, **opts):
        """The cascade `plan` over the batch `name` under the options `opts` (restored afterwards): (host arrays,
        per-pass statistics)."""
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
def rig(native_lib, oracle_lib):
    r = Rig()
    yield r
    r.close()


def check(route, rig, name, policy, host, stats, k, poly_t=0, tail=False):
    """Pass k of the run against the scan: every read's (entry, offset, mismatches), unclaimed where the scan found
    nothing, processed / aligned; a decoy pass in front claimed nothing.  tail: the `-v 0` pass behind pass k may claim
    what pass k left -- under a poly-T rule the reads the rule keeps out (a run of two T the entry happens to continue
    with): then exactly what the scan of the whole reads says."""
    sw = rig.sweeps[name]
    scan, processed = ws.scan_answers(sw, policy, poly_t)
    got = es.claimed(*host, k)
    report = es.grid_report("%s on %s" % (route, name), policy, sw.cases, got, scan)
    assert not report, report
    aligned = int((scan[:, 0] >= 0).sum())
    if tail:
        rest = np.array(es.scan_answers(sw, es.EXACT_POLICIES[1]))
        rest[scan[:, 0] >= 0] = -1
        report = es.grid_report("%s on %s, the `-v 0` pass behind" % (route, name), policy, sw.cases, es.claimed(*host, k + 1), rest)
        assert not report, report
        assert (stats[k + 1]["processed"], stats[k + 1]["aligned"]) == (len(sw.cases) - aligned, int((rest[:, 0] >= 0).sum())), (route, name, policy)
    assert set(np.unique(host[0]).tolist()) <= ({k, k + 1, -1} if tail else {k, -1}), (route, name, policy)
    for i in range(k):
        assert (stats[i]["processed"], stats[i]["aligned"]) == (len(sw.cases), 0), (route, name, policy, i)
    assert (stats[k]["processed"], stats[k]["aligned"]) == (processed, aligned), (route, name, policy)
    print("%s on %s, policy %s: %d reads compared, %d aligned; lds_mode %d, variant %d, pair_anchor %d, launches %d" %
          (route, name, policy, len(sw.cases), stats[k]["aligned"], stats[k]["lds_mode"], stats[k]["variant"], stats[k]["pair_anchor"],
           stats[k]["n_launches"]))


def plan_of(policy, decoy=False, tail=False, poly_t=0):
    """The policy on the sweep's library; behind the decoy pass; with a `-v 0` pass on the same library behind it (it only
    gives a fused launch its second member: what it could claim, every policy of the sweep has claimed)."""
    return ([DECOY] if decoy else []) + [ws.pass_dict(policy, "lib", poly_t)] + ([es.pass_dict(es.EXACT_POLICIES[1], "lib")] if tail else [])


FM = dict(dict=(0, 1))      # no dictionary kernels, no split: the whole batch, W words per read, in the FM kernels


@pytest.mark.parametrize("W", WORDS)
def test_route_1_a_pass_alone_in_match_kernel(rig, W):
    """match_kernel<W> for the four policies with at most one seed mismatch; the 2-mismatch policy in stratum_kernel<W>
    over the anchor pairs, with `pair_seeds` = 0 its strata in match_kernel<W>, with `stratum_rows` = 2 on top its
    pigeonhole pieces in stratum_kernel<W>."""
    name = "w%d" % W
    for policy in es.POLICIES:
        host, st = rig.run(name, plan_of(policy), **FM)
        if policy[1] == 2:
            assert st[0]["lds_mode"] in STRATUM and st[0]["pair_anchor"] == 4 and st[0]["n_launches"] == 1, st[0]
        else:
            assert st[0]["lds_mode"] in MATCH and st[0]["n_launches"] == 1, st[0]
        check("route 1 (%s<%d> alone)" % ("stratum_kernel" if policy[1] == 2 else "match_kernel", W), rig, name, policy, host, st, 0)
    host, st = rig.run(name, plan_of(es.TWO_MM_POLICY), pair_seeds=(0, 1), **FM)
    assert st[0]["lds_mode"] in MATCH and st[0]["pair_anchor"] == 0 and st[0]["n_launches"] == 2, st[0]
    check("route 1 (match_kernel<%d>, strata)" % W, rig, name, es.TWO_MM_POLICY, host, st, 0)
    host, st = rig.run(name, plan_of(es.TWO_MM_POLICY), pair_seeds=(0, 1), stratum_rows=(2, 0), **FM)
    assert st[0]["lds_mode"] in STRATUM and st[0]["pair_anchor"] == 0 and st[0]["n_launches"] == 2, st[0]
    check("route 1 (stratum_kernel<%d>, pieces)" % W, rig, name, es.TWO_MM_POLICY, host, st, 0)


@pytest.mark.parametrize("W", WORDS)
def test_route_2_fused_kernel(rig, W):
    """The policy between the decoy pass and a `-v 0` pass on its own library runs in fused_kernel<W>; the same plan
    with `fuse` = 0 in match_kernel<W> behind a survivor list."""
    name = "w%d" % W
    for policy in es.POLICIES[:4]:
        host, st = rig.run(name, plan_of(policy, decoy=True, tail=True), **FM)
        assert st[0]["lds_mode"] in MATCH and st[1]["lds_mode"] in FUSED and st[2]["lds_mode"] in FUSED and st[2]["group"] == 1, st
        check("route 2 (fused_kernel<%d>)" % W, rig, name, policy, host, st, 1)
        host, st = rig.run(name, plan_of(policy, decoy=True, tail=True), fuse=(0, 1), **FM)
        assert st[1]["lds_mode"] in MATCH and st[1]["group"] == 1 and st[2]["group"] == 2, st
        check("route 2 (match_kernel<%d> behind a list)" % W, rig, name, policy, host, st, 1)


@pytest.mark.parametrize("mode", (0, 1, 2, 3))
def test_route_3_every_residency_of_match_kernel(rig, mode):
    """`force_lds_mode`: match_kernel<2, blocks, text> with nothing, the occ blocks, both, the text in LDS."""
    for policy in (es.EXACT_POLICIES[1], es.ONE_MM_POLICIES[0]):
        host, st = rig.run("w2", plan_of(policy), force_lds_mode=(mode, -1))
        assert st[0]["lds_mode"] == mode and st[0]["n_launches"] == 1, st[0]
        check("route 3 (match_kernel<2>, force_lds_mode %d)" % mode, rig, "w2", policy, host, st, 0)


@pytest.mark.parametrize("W", WORDS)
def test_route_4_the_split_batch(rig, W):
    """Default options: the batch -- one-word reads without N, one-word reads with N, reads beyond 32 nt (W = 2: of
    33..64 nt) -- runs as two cascades, its one-word N-free reads in the dictionary kernels' lane (the kernel the
    statistics name) and the rest in the FM kernels: pass 0 reports two launches and every read equals the scan,
    whichever lane took it.  With `split_mixed` = 0 the whole batch runs in the FM kernels, one launch."""
    name = "w%d" % W
    sw = rig.sweeps[name]
    lane = sum(1 for c in sw.cases if c.L <= 32 and "N" not in c.read)
    assert lane > 1000 and sum(1 for c in sw.cases if c.L <= 32 and "N" in c.read) > 1000 and sum(1 for c in sw.cases if c.L > 32) > 1000
    for policy in es.POLICIES:
        host, st = rig.run(name, plan_of(policy))
        want = EXACT if policy[1] == 0 else PAIR_WAVE if policy[1] == 2 else MATCH
        assert st[0]["lds_mode"] in want and st[0]["n_launches"] == 2 and st[0]["ms_rest"] > 0, st[0]
        check("route 4 (split batch, %d reads in the one-word lane)" % lane, rig, name, policy, host, st, 0)
        host, st = rig.run(name, plan_of(policy), split_mixed=(0, 1))
        assert st[0]["lds_mode"] in (STRATUM if policy[1] == 2 else MATCH) and st[0]["n_launches"] == 1 and st[0]["ms_rest"] == 0, st[0]
        check("route 4 (split_mixed 0)", rig, name, policy, host, st, 0)


@pytest.mark.parametrize("seed_impl", (-1, 2))
def test_route_5_the_long_lane(rig, seed_impl):
    """`long_lane` = 1: the N-free reads of 33..63 nt of the W = 2 batch ride the one-word lane.  Behind the decoy the
    four policies with at most one seed mismatch run in the seed launch's LONG instantiation (`variant` & 8; seed_kernel
    by default, wave_seed_kernel with `seed_impl` = 2); the 2-mismatch policy in pair_wave_kernel's, whose window
    admits the reads of 33..35 nt behind `-5 1 -3 2` (the longer ones stay with the FM kernels).  The poly-T class too:
    its 2-mismatch policy has no anchor pairs and hence no LONG instantiation to run in."""
    sw = rig.sweeps["w2"]
    assert sum(1 for c in sw.cases if 33 <= c.L <= 63 and "N" not in c.read) > 1000
    kernel = "wave_seed_kernel" if seed_impl == 2 else "seed_kernel"
    for name, poly_t in (("w2", 0), ("w2_polyt", 1)):
        for policy in es.POLICIES:
            host, st = rig.run(name, plan_of(policy, decoy=True, poly_t=poly_t), long_lane=(1, 0), seed_impl=(seed_impl, -1))
            if policy[1] < 2:
                assert st[1]["lds_mode"] in SEED and st[1]["variant"] & LONG and st[1]["variant"] & 3 == (2 if seed_impl == 2 else 0), st[1]
                route = "route 5 (%s, LONG%s)" % (kernel, ", poly_t" if poly_t else "")
            elif not poly_t:
                assert st[1]["lds_mode"] in PAIR_WAVE and st[1]["variant"] & LONG and st[1]["pair_anchor"] == 4, st[1]
                route = "route 5 (pair_wave_kernel, LONG)"
            else:
                assert st[1]["lds_mode"] in MATCH + STRATUM, st[1]
                route = "route 5 (2 mismatches, poly_t: FM kernels)"
            check(route, rig, name, policy, host, st, 1, poly_t)


@pytest.mark.parametrize("W", WORDS)
def test_route_6_the_poly_t_class_in_the_fm_kernels(rig, W):
    """`poly_t` = 1, the T tail walked over W words and the N mask by each kernel's own code: a pass alone in
    match_kernel<W> (the 2-mismatch policy: its strata, two launches -- the anchor pairs do not take a poly-T pass -- and
    with `stratum_rows` = 2 in stratum_kernel<W>), and between the decoy and a `-v 0` pass in fused_kernel<W>."""
    name = "w%d_polyt" % W
    for policy in es.POLICIES:
        host, st = rig.run(name, plan_of(policy, poly_t=1), **FM)
        assert st[0]["lds_mode"] in MATCH and st[0]["pair_anchor"] == 0 and st[0]["n_launches"] == (2 if policy[1] == 2 else 1), st[0]
        check("route 6 (poly_t, match_kernel<%d>)" % W, rig, name, policy, host, st, 0, poly_t=1)
    host, st = rig.run(name, plan_of(es.TWO_MM_POLICY, poly_t=1), stratum_rows=(2, 0), **FM)
    assert st[0]["lds_mode"] in STRATUM and st[0]["pair_anchor"] == 0 and st[0]["n_launches"] == 2, st[0]
    check("route 6 (poly_t, stratum_kernel<%d>)" % W, rig, name, es.TWO_MM_POLICY, host, st, 0, poly_t=1)
    for policy in es.POLICIES[:4]:
        host, st = rig.run(name, plan_of(policy, decoy=True, tail=True, poly_t=1), **FM)
        assert st[1]["lds_mode"] in FUSED and st[2]["lds_mode"] in FUSED and st[2]["group"] == 1, st
        check("route 6 (poly_t, fused_kernel<%d>)" % W, rig, name, policy, host, st, 1, poly_t=1, tail=True)
