"""Predict mode's classification without a GPU: the reader of the model files (mirge_amd/svm_model.py) on pickles the test
writer makes, every refusal included; the native reader of the screened table and its writers (csrc/predict_model_write.cpp)
on the fixture's worlds -- the three filter files against the reference's byte for byte, the feature rows against the rule's,
the two result files from the rule's numbers -- and the repr formatting, the header-only table, the thread and block
independence and the refusals."""
import ctypes as C
import os

import numpy as np
import pytest

from mirge_amd import predict, svm_model
from tests import predict_model_cases as cases
from tests import predict_model_model as rule

GOLD = cases.golden()
WORLDS = {w["name"]: w for w in GOLD["worlds"]}
NAMELIST = GOLD["namelist"]


@pytest.fixture(scope="module")
def lib(native_lib):
    from mirge_amd import _native
    return _native.load()


@pytest.fixture(scope="module")
def model():
    return cases.fixture_model()


@pytest.fixture(scope="module")
def world_results(model):
    """name -> (table text, the rule's results), computed once."""
    out = {}
    for name in WORLDS:
        text = cases.world_text(model, name)
        out[name] = (text, rule.run(text, NAMELIST, model))
    return out


def same_model(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a[:4], b[:4])) and a[4:] == b[4:]


# ------------------------------------------------------------------------------------------------ the reader
@pytest.mark.parametrize("nf,n_sv", [(1, 1), (12, 65), (21, 130), (64, 3)])
def test_reader_returns_the_arrays_written(nf, n_sv):
    m = cases.hand_model(nf, n_sv)
    got = svm_model.parse_model(cases.model_file_bytes(m))
    assert same_model(got, m)
    assert got.sv.shape == (n_sv, nf) and got.coef.shape == (n_sv,) and got.sv.dtype == np.float64


def test_reader_returns_the_fixture_model(model, tmp_path):
    d = cases.write_model_dir(str(tmp_path / "models"), model, "human")
    assert same_model(svm_model.load_model(d, "human"), model)
    assert svm_model.read_namelist(d) == [n.strip() for n in NAMELIST]
    cases.write_model_dir(d, cases.hand_model(3, 4), "others")
    assert svm_model.load_model(d, "zebrafish").sv.shape == (4, 3)      # every other species takes `others`
    assert svm_model.model_path(d, "mouse").endswith("mouse_svc_model.pkl")
    with pytest.raises(OSError):
        svm_model.load_model(d, "mouse")


def test_reader_turns_fortran_order_back_and_reads_numpys_own_pickles():
    m = cases.hand_model(5, 7)
    plain = svm_model.parse_model(cases.model_file_bytes(m))
    for variation in (dict(sv_order="F"), dict(inline=True), dict(sv_order="F", inline=True)):
        raw = cases.model_file_bytes(m, **variation)
        assert raw != cases.model_file_bytes(m)
        got = svm_model.parse_model(raw)
        assert same_model(got, m) and same_model(got, plain) and got.sv.shape == (7, 5)


def test_reader_refuses_an_object_that_never_got_its_state():
    with pytest.raises(svm_model.ModelError) as e:
        svm_model.parse_model(cases.model_file_bytes(cases.hand_model(5, 7), state=False), "the file")
    assert "no field kernel" in str(e.value)


def test_reader_bounds_what_a_file_inflates_to(monkeypatch):
    raw = cases.model_file_bytes(cases.hand_model(5, 7))
    monkeypatch.setattr(svm_model, "MAX_PICKLE_BYTES", 100)
    with pytest.raises(svm_model.ModelError, match="larger than 100 bytes"):
        svm_model.parse_model(raw)


def test_tolerance_of_the_fixture_model(model):
    assert float(GOLD["tolerance"]) == rule.tolerance(model)
    assert 1e-9 < rule.tolerance(model) < 1e-8


REFUSALS = [
    (dict(extra_global=("os", "system")), "os.system"),
    (dict(extra_global=("builtins", "eval")), "builtins.eval"),
    (dict(extra_global=("sklearn.svm.classes", "LinearSVC")), "sklearn.svm.classes.LinearSVC"),
    (dict(kernel="linear"), "kernel"),
    (dict(classes=(-1, 0, 1)), "classes_"),
    (dict(classes=(0, 1)), "classes_"),
    (dict(probability=False), "probability"),
    (dict(sparse=True), "_sparse"),
    (dict(with_mean=False), "with_mean"),
    (dict(steps=2), "steps"),
]


@pytest.mark.parametrize("variation,word", REFUSALS)
def test_reader_refuses(variation, word):
    m = cases.hand_model(5, 6)
    with pytest.raises(svm_model.ModelError) as e:
        svm_model.parse_model(cases.model_file_bytes(m, **variation), "the file")
    assert word in str(e.value) and "the file" in str(e.value)


def test_reader_refuses_shapes_that_disagree():
    m = cases.hand_model(5, 6)
    for bad, word in ((m._replace(coef=m.coef[:-1]), "dual_coef_"), (m._replace(mean=m.mean[:-1]), "mean_"),
                      (m._replace(feature_names=m.feature_names[:-1]), "selected features"),
                      (cases.hand_model(65, 2), "features")):
        with pytest.raises(svm_model.ModelError) as e:
            svm_model.parse_model(cases.model_file_bytes(bad, coef_shape=(1, len(bad.coef))))
        assert word in str(e.value)
    with pytest.raises(svm_model.ModelError):
        svm_model.parse_model(b"not a zlib stream")
    whole = cases.model_file_bytes(m)
    import zlib
    with pytest.raises(svm_model.ModelError):
        svm_model.parse_model(zlib.compress(zlib.decompress(whole)[:-40]))


# ------------------------------------------------------------------------------------------------ the worlds
def write_table(tmp_path, text):
    path = str(tmp_path / cases.TABLE)
    with open(path, "w") as fh:
        fh.write(text)
    return path


def read(path):
    with open(path) as fh:
        return fh.read()


def test_output_names(tmp_path):
    path = str(tmp_path / cases.TABLE)
    assert predict.classified_paths(path) == rule.output_paths(path)
    assert os.path.basename(predict.classified_paths(path)["novel"]) == "smp_novel_miRNAs_miRge2.0.csv"


@pytest.mark.parametrize("name", sorted(WORLDS))
def test_world_filters_rows_and_result_files(lib, model, world_results, tmp_path, name):
    text, want = world_results[name]
    world = WORLDS[name]
    assert cases.text_digest(text) == world["sha256"]
    path = write_table(tmp_path, text)
    with predict.ScreenedTable(path, model, NAMELIST) as table:
        for key in ("dataset", "refined_tmp", "refined"):
            got = read(table.paths[key])
            assert got == want[key]
            assert cases.text_digest(got) == world["files"][key]          # the reference's file, byte for byte
        assert table.rows == (text.count("\n") - 1, want["dataset"].count("\n") - 1, len(want["x"]))
        assert table.stray == len(want["stray"]) == (1 if name == "stray" else 0)
        assert table.x.shape == want["x"].shape and np.array_equal(table.x, want["x"])
        predicted, kept = table.write(want["pred"], want["prob"])
        detailed, novel = read(table.paths["detailed"]), read(table.paths["novel"])
    assert detailed == want["detailed"] and novel == want["novel"]
    assert predicted == int((want["pred"] == 1).sum()) and kept == len(world["novel"]) == novel.count("\n") - 1
    # ... and against the reference's own: labels and order as text, probabilities within the margin
    margin = cases.prob_margin(model, rule.tolerance(model))
    lines = detailed.splitlines()[1:]
    assert len(lines) == len(world["rows"])
    for ln, ref in zip(lines, world["rows"]):
        c, r = ln.split(","), ref.split(",")
        assert c[0] == r[0] and abs(float(c[1]) - float(r[1])) <= margin
    assert [lines.index(ln) for ln in novel.splitlines()[1:]] == world["novel"]


def test_worlds_hold_what_the_maker_asserted():
    held = set(h for w in WORLDS.values() for h in w["holds"])
    for what in ("clip", "clip_high", "clip_low", "kept", "predicted_1_below_cutoff", "predicted_1_with_larger_probability_of_minus_1", "rounds_0", "rounds_1", "rounds_2",
                 "count_below_10", "fewer_than_3_sequences", "cell_equal_N", "cell_containing_N", "none_structure", "selected_name_absent",
                 "stray_string"):
        assert what in held
    assert all(len(w["dropped"]) <= 0.01 * (len(w["rows"]) + len(w["dropped"])) for w in WORLDS.values())


def test_bytes_do_not_depend_on_threads_or_block(lib, model, world_results, tmp_path, monkeypatch):
    text, want = world_results["main"]
    path = write_table(tmp_path, text)
    monkeypatch.setenv("MIRGE_AMD_MODEL_BLOCK_LINES", "7")
    with predict.ScreenedTable(path, model, NAMELIST) as table:
        table.write(want["pred"], want["prob"], threads=3)
        assert read(table.paths["detailed"]) == want["detailed"] and read(table.paths["novel"]) == want["novel"]


def test_kept_row_whose_larger_probability_is_class_minus_1s(lib, model, world_results, tmp_path):
    """model_predict.py:63 prints max() over both classes: a row predicted 1 with 0.9 for class -1 is kept; ties in the
    probability are ordered by the line's text, descending."""
    text, want = world_results["absent"]
    path = write_table(tmp_path, text)
    n = len(want["x"])
    pred = np.full(n, -1, np.int8)
    prob = np.tile([0.9, 0.1], (n, 1))
    pred[[2, 5, 7]] = 1
    prob[5] = (0.1, 0.9)
    prob[7] = (0.21, 0.79)
    with predict.ScreenedTable(path, model, NAMELIST) as table:
        assert table.write(pred, prob) == (3, 2)
        novel = read(table.paths["novel"]).splitlines()
    names = [",".join(r) for r in want["names_of_rows"]]
    assert novel[1:] == sorted(["1,0.9," + names[2], "1,0.9," + names[5]], reverse=True)
    assert rule.result_texts(novel[0].split(",")[2:], want["names_of_rows"], pred, prob)[1].splitlines() == novel


def test_header_only_table(lib, model, tmp_path):
    path = write_table(tmp_path, cases.header_only_text())
    with predict.ScreenedTable(path, model, NAMELIST) as table:
        assert table.rows == (0, 0, 0) and table.x.shape == (0, 21) and table.stray == 0
        assert table.write(np.zeros(0, np.int8), np.zeros((0, 2))) == (0, 0)
        want = rule.filter_texts(cases.header_only_text(), NAMELIST)
        assert [read(table.paths[k]) for k in ("dataset", "refined_tmp", "refined")] == list(want)
        assert all(t.count("\n") == 1 for t in want)
        head = "predictedValue,probability,realMicRNA,realMicRNAName,clusterName\n"
        assert read(table.paths["detailed"]) == head and read(table.paths["novel"]) == head


@pytest.mark.parametrize("text,word", [
    ("", "no header"),
    ("a\tb\tc\n", "readCountSum"),
    ("\t".join(h for h in cases.HEADER if h != "pruned_precusor_str") + "\n", "pruned_precusor_str"),
])
def test_tables_that_are_refused(lib, model, tmp_path, text, word):
    from mirge_amd._native import MirgeAmdError
    path = write_table(tmp_path, text)
    with pytest.raises(MirgeAmdError) as e:
        predict.ScreenedTable(path, model, NAMELIST)
    assert word in str(e.value) and e.value.code == -1
    assert not os.path.exists(predict.classified_paths(path)["dataset"])     # nothing is written


def test_count_that_is_no_whole_number(lib, model, tmp_path):
    from mirge_amd._native import MirgeAmdError
    rows = cases.world_rows(model, "stray", 3, 1)
    rows[1]["readCountSum"] = "12.5"
    with pytest.raises(MirgeAmdError) as e:
        predict.ScreenedTable(write_table(tmp_path, cases.table_text(rows)), model, NAMELIST)
    assert "line 2" in str(e.value)


# ------------------------------------------------------------------------------------------------ repr
def test_repr_formatting(lib):
    rng = np.random.default_rng(3)
    values = [0.0, -0.0, 0.5, 0.8, 0.79999973, 1.0 - 1e-7, 1e-7, 1.0, 0.1, 0.3, 2.0 / 3.0, 1e16, 1e15, 123456789012345680.0, 9999999999999998.0,
              1e-4, 0.0001234, 9.999e-5, 1e-5, 5e-324, 1.7976931348623157e308, 2.2250738585072014e-308, -1.5, -1e-10, 1e22, 1e23, 100.0,
              0.7999999999999999, 0.8000000000000002, 0.9999999, float("inf"), float("-inf")]
    values += list(rng.uniform(0.5, 1.0, 300)) + list(np.exp(rng.uniform(-40, 40, 300))) + [float(np.nextafter(0.8, 0)), float(np.nextafter(0.8, 1))]
    buf = C.create_string_buffer(64)
    for v in values:
        assert lib.mrg_format_repr(float(v), buf, 64) == 0
        assert buf.value.decode() == repr(float(v)), repr(float(v))
    assert lib.mrg_format_repr(float("nan"), buf, 64) == 0 and buf.value == b"nan"
    assert lib.mrg_format_repr(0.1, buf, 3) == -1
