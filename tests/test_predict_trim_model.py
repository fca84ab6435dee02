"""tests/predict_trim_model.py against the reference's own output (tests/golden/predict_trim.json, captured by
tests/golden/make_predict_trim_golden.py from preTrimClusteredSeq.py and generate_Seq.py): byte for byte on every world
without ties; on the world with ties on every row whose outcome does not depend on the order among equal distances.  And
the choice of the two nearest elements against scipy's cKDTree and against a plain sort."""
import json
import os

import numpy as np
import pytest

from tests import predict_trim_model as model

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "predict_trim.json")


def worlds():
    with open(GOLDEN) as fh:
        return json.load(fh)["worlds"]


WORLDS = worlds()


def test_the_fixture_covers_what_it_should():
    names = [w["name"] for w in WORLDS]
    assert len(names) >= 10 and names.count("ties") == 1 and "empty" in names
    assert sum(not w["ties"] for w in WORLDS) >= 9
    tsv = "".join(w["trimmed_tsv"] for w in WORLDS)
    assert "\t+\t" in tsv and "\t-\t" in tsv and "N" in tsv and "\t0\t*\t" in tsv and "\t1\t*\t" in tsv and "\t0\tgiant\t" in tsv
    assert os.path.getsize(GOLDEN) < 1 << 20


@pytest.mark.parametrize("w", [w for w in WORLDS if not w["ties"]], ids=lambda w: w["name"])
def test_model_equals_the_reference_byte_for_byte(w):
    # no row of these worlds depends on the order among equal distances: the reference alone fixes them
    assert model.outcomes(w["table"], w["elements"], w["cutoff"]) == model.outcomes(w["table"], w["elements"], w["cutoff"], True)
    tsv, fa, fo = model.files(w["table"], w["elements"], w["cutoff"])
    assert tsv == w["trimmed_tsv"]
    assert fa == w["trimmed_fa"]
    assert fo == w["trimmed_orig_fa"]


def test_the_empty_table_is_a_header_and_two_empty_files():
    w = next(w for w in WORLDS if w["name"] == "empty")
    assert w["trimmed_tsv"].count("\n") == 1 and w["trimmed_tsv"].startswith(model.HEADER_HEAD + "\tChr\t")
    assert w["trimmed_fa"] == "" and w["trimmed_orig_fa"] == ""


def test_ties_world_equals_the_reference_where_the_order_does_not_matter():
    w = next(w for w in WORLDS if w["ties"])
    low = model.outcomes(w["table"], w["elements"], w["cutoff"])
    high = model.outcomes(w["table"], w["elements"], w["cutoff"], high_first=True)
    same = [i for i in range(len(low)) if low[i] == high[i]]
    assert 0 < len(low) - len(same) and len(same) >= 0.9 * len(low)
    got = model.parse_table(model.files(w["table"], w["elements"], w["cutoff"])[0])[1]
    ref = model.parse_table(w["trimmed_tsv"])[1]
    assert len(got) == len(ref) == len(low)
    for i in same:
        assert got[i] == ref[i], i
    # the choice itself, on the hand-made rows: the lower start first, then the lower index
    assert low[0] == ("0", "a") and high[0] == ("1", "*")


def test_nearest_two_equals_a_plain_sort_ties_included():
    rng = np.random.default_rng(5)
    for _ in range(300):
        n = int(rng.integers(0, 12))
        start = sorted(int(x) for x in rng.integers(1, 30, n))     # (many equal starts, many equal distances)
        lo = int(rng.integers(0, n + 1))
        hi = int(rng.integers(lo, n + 1))
        at = int(rng.integers(0, 32))
        for high in (False, True):
            assert model.nearest_two(start, lo, hi, at, high) == model.nearest_two_brute(start, lo, hi, at, high)


def test_nearest_two_equals_ckdtree_without_ties():
    cKDTree = pytest.importorskip("scipy.spatial").cKDTree
    rng = np.random.default_rng(6)
    done = 0
    while done < 300:
        n = int(rng.integers(2, 200))
        file_order = rng.choice(np.arange(1, 5000), size=n, replace=False)
        tree = cKDTree([(int(s), 0) for s in file_order])
        order = np.argsort(file_order, kind="stable")
        start = [int(file_order[k]) for k in order]
        for at in rng.integers(1, 5200, 10):
            at = int(at)
            two = model.nearest_two(start, 0, n, at)
            if two != model.nearest_two(start, 0, n, at, high_first=True):
                continue
            _, idx = tree.query([(at, 0)], 2)
            assert [int(order[k]) for k in two] == [int(idx[0][0]), int(idx[0][1])]
            done += 1


def test_flat_repeats_sorts_stably_and_drops_unknown_entries():
    rep_off, start, end, name_id, names = model.flat_repeats(
        ["chrB", "chrA", "chrC"], {"chrA": [(9, 10, "x"), (5, 6, "y"), (9, 1, "z"), (5, 7, "x")], "chrQ": [(1, 2, "q")]})
    assert rep_off == [0, 0, 4, 4] and start == [5, 5, 9, 9] and end == [6, 7, 10, 1]
    assert [names[k] for k in name_id] == ["y", "x", "x", "z"] and "q" not in names
