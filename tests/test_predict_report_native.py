"""Predict mode's report without a GPU: the native reader of the three files (csrc/predict_report_write.cpp) against the rule's
arrays, and the native writers fed the rule's arrays -- `_corrected.tsv` and the report against the reference's own files from
tests/golden/predict_report.json, the profile file against the reference's recorded creatPDF arguments and the rule's sums --
for every world; the raising cases; the refusals; and the independence of thread count and block size."""
import os

import numpy as np
import pytest

from mirge_amd import predict
from tests import predict_report_cases as cases
from tests import predict_report_model as rule

GOLD = {w["name"]: w for w in cases.golden()["worlds"]}


@pytest.fixture(scope="module")
def lib(native_lib):
    from mirge_amd import _native
    return _native.load()


@pytest.fixture(scope="module")
def worlds():
    """name -> (the three texts, the rule's results), computed once."""
    out = {}
    for name in cases.WORLDS:
        texts = cases.world(name)
        out[name] = (texts, rule.run(*texts))
    return out


def write_inputs(d, texts):
    paths = [os.path.join(str(d), nm) for nm in (cases.NOVEL, cases.TABLE, cases.CLUSTER)]
    for p, text in zip(paths, texts):
        with open(p, "w") as fh:
            fh.write(text)
    return paths


def read(path):
    with open(path) as fh:
        return fh.read()


def check_against_fixture(name, texts, files):
    """files: corrected / report / profiles texts of a run over `texts`."""
    gold = GOLD[name]
    keep = (lambda s: s) if gold["as_text"] else cases.digest
    assert [keep(s) for s in texts] == gold["inputs"], "the generator no longer makes the world the reference ran on"
    assert keep(files["corrected"]) == gold["corrected"]
    assert keep(files["report"]) == gold["report"]
    # the profile file: the rows the reference handed to creatPDF, in its order, and its scalars
    assert cases.calls_digest(cases.calls_form_from_files(files["report"], files["profiles"])) == gold["calls_sha256"]
    blocks = files["profiles"].split(">")[1:]
    assert len(blocks) == gold["n_calls"]
    for k, block in enumerate(blocks):
        ls = block.split("\n")
        head = ls[0].split("\t")
        rows = [[t, int(c)] for t, c in (ln.split("\t") for ln in ls[4:-1])]
        if gold["as_text"]:   # ... and call by call where the fixture keeps them
            call = gold["calls"][k]
            assert rows == call["mature_rows"] + ([] if call["passenger_rows"] == "None" else call["passenger_rows"])
            assert head[0] == call["name"] and ls[1] == call["precursor"] and ls[2] == call["structure"]
        assert int(head[1]) == len(ls[1]) and int(head[3]) == len(rows) and int(head[2]) == sum(r[1] for r in rows)
        sums, total, ragged = rule.profile_of(ls[1], [(r[0], r[1]) for r in rows])
        assert ls[3] == "\t".join(str(s) for s in sums) and int(head[4]) == ragged
        assert ls[-1] == ""


def test_the_fixture_holds_what_it_must():
    held = set()
    for w in GOLD.values():
        held |= set(w["holds"])
    for case in ("offer_upstream", "offer_downstream", "both_offers_to_one_line", "first_line_offers_to_header", "retyped_to_loop",
                 "already_loop", "cluster_seq_absent", "close_before_open_only", "group_of_5", "both_listed_tie", "only_second_listed",
                 "passenger_dropped_for_loop", "mature_loop_skipped", "strand_minus", "negative_pad", "ragged_row", "repeated_name_in_list"):
        assert case in held


@pytest.mark.parametrize("name", cases.WORLDS)
def test_reader_gives_the_rules_arrays(lib, worlds, name, tmp_path):
    texts, _ = worlds[name]
    want = rule.arrays(*texts)
    with predict.ReportInputs(*write_inputs(tmp_path, texts)) as inputs:
        assert (inputs.n, inputs.n_listed, inputs.n_rows) == (want["n"], want["n_listed"], len(want["row_start"]))
        for key in predict.REPORT_ARRAYS:
            mine = np.frombuffer(want[key], np.uint8) if isinstance(want[key], bytes) else want[key].reshape(-1)
            assert inputs.arrays[key].dtype == mine.dtype and np.array_equal(inputs.arrays[key], mine), key


@pytest.mark.parametrize("name", cases.WORLDS)
def test_writers_give_the_references_files(lib, worlds, name, tmp_path):
    texts, res = worlds[name]
    with predict.ReportInputs(*write_inputs(tmp_path, texts)) as inputs:
        inputs.write(res)
        files = {key: read(p) for key, p in inputs.paths.items()}
    assert files == {key: res[key] for key in files}
    check_against_fixture(name, texts, files)
    if name == "nothing_listed":
        assert files["report"] == rule.REPORT_HEADER and files["profiles"] == "" and files["corrected"] == texts[1]


def test_paths_are_the_references(tmp_path):
    paths = write_inputs(tmp_path, cases.world("nothing_listed"))
    got = predict.report_paths(*paths)
    assert got == rule.output_paths(*paths)
    assert os.path.basename(got["report"]) == "smp_novel_miRNAs_report.csv"
    assert got["corrected"].endswith("_updated_stableClusterSeq_15_corrected.tsv")


@pytest.mark.parametrize("threads,block", [(1, 1), (3, 2), (16, 7)])
def test_files_do_not_depend_on_threads_or_blocks(lib, worlds, threads, block, tmp_path, monkeypatch):
    texts, res = worlds["random_a"]
    monkeypatch.setenv("MIRGE_AMD_REPORT_BLOCK_LINES", str(block))
    with predict.ReportInputs(*write_inputs(tmp_path, texts)) as inputs:
        inputs.write(res, threads=threads)
        for key, p in inputs.paths.items():
            assert read(p) == res[key], key


@pytest.mark.parametrize("name", sorted(cases.raising_cases()))
def test_raising_cases(lib, name, tmp_path):
    """The rule raises where the reference does; the reader itself takes these files (the device finds the case), and a writer
    handed the arrays of a stage that had gone on regardless refuses what it can see and leaves no file."""
    texts = cases.raising_cases()[name]
    with pytest.raises(ValueError):
        rule.run(*texts)
    with predict.ReportInputs(*write_inputs(tmp_path, texts)) as inputs:
        n = inputs.n
        unlisted = [j for j in range(n) if not inputs.arrays["flags"][j] & 1]
        if unlisted:   # an entry whose mature line nobody listed
            m = unlisted[0]
            L = len(inputs.strings(m)[0])
            rows = len(inputs.rows(m))
            res = dict(n_entries=1, src=np.arange(n), state=np.zeros(n), pos_adj=np.zeros((n, 2)), ent_m=[m], ent_p=[-1], row_off=[0, rows],
                       prof_off=[0, L], lead=np.zeros(rows), trail=np.zeros(rows), prof=np.zeros(L), total=[0], flag=[0])
            with pytest.raises(ValueError):
                inputs.write(res)
        res = dict(n_entries=0, src=np.arange(n) + 2, state=np.zeros(n), pos_adj=np.zeros((n, 2)), ent_m=[], ent_p=[], row_off=[0], prof_off=[0],
                   lead=[], trail=[], prof=[], total=[], flag=[])
        with pytest.raises(ValueError):   # src names no neighbour
            inputs.write(res)
        assert not any(os.path.exists(p) for p in inputs.paths.values())


def test_reader_refuses_malformed_files(lib, tmp_path):
    novel, table, cluster = cases.world("hand")

    def refused(texts, word):
        with pytest.raises(ValueError) as e:
            predict.ReportInputs(*write_inputs(tmp_path, texts))
        assert word in str(e.value), str(e.value)
    refused((novel, table.replace("pruned_precusor_str", "pruned_str", 1), cluster), "no column pruned_precusor_str")
    refused((novel, table.replace("upstreamDistance", "up", 1), cluster), "no column upstreamDistance")
    refused((novel.replace("clusterName", "name", 1), table, cluster), "no column clusterName")
    refused((novel.replace("probability", "p", 1), table, cluster), "no column probability")
    refused(("", table, cluster), "no header line")
    refused((novel, "", cluster), "no header line")
    header = table.split("\n")[0].split("\t")
    name = table.split("\n")[1].split("\t")[header.index("clusterName")]
    for bad in (name[:-1], name.replace(":chr1:", ":chr1:x:"), name.replace("_", "-"), name.replace(":1000_", ":10a0_")):
        refused((novel, table.replace(name, bad), cluster), "clusterName is not")
    lines = table.split("\n")
    refused((novel, "\n".join(lines[:3] + [lines[2]] + lines[3:]), cluster), "clusterName is repeated")
    refused((novel, "\n".join(lines[:2] + ["\t".join(lines[2].split("\t")[:-1])] + lines[3:]), cluster), "fewer cells")
    refused((novel + "1,0.9,Null,Null,smp:miRCluster_999_22:chr1:5_26+\n", table, cluster), "which the table does not hold")
    cells = lines[2].split("\t")
    cells[header.index("readCountSum")] = "many"
    refused((novel, "\n".join(lines[:2] + ["\t".join(cells)] + lines[3:]), cluster), "no whole number")
    from mirge_amd._native import MirgeAmdError
    with pytest.raises(MirgeAmdError):   # (a file that cannot be opened is the library's I/O error)
        predict.ReportInputs(str(tmp_path / "absent.csv"), str(tmp_path / "absent.tsv"), str(tmp_path / "absent.txt"))


def test_a_missing_or_malformed_block_is_marked_not_refused(lib, tmp_path):
    """The reference reads a block only when it needs it: the reader marks it, the entry pass raises when an entry names it."""
    novel, table, cluster = cases.world("hand")
    blocks = cluster.split("Cluster Name: ")[1:]
    bent = "Cluster Name: " + "Cluster Name: ".join([blocks[0].replace("\t50\n", "\tfifty\n")] + blocks[2:])
    with predict.ReportInputs(*write_inputs(tmp_path, (novel, table, bent))) as inputs:
        assert inputs.arrays["blk"][:3].tolist() == [2, 0, 1]
        assert inputs.rows(0) == [] and inputs.rows(1) == [] and len(inputs.rows(2)) == 3


def test_host_restatements_agree_with_the_rule(worlds):
    """predict.host_report_line / host_report_entry, the route of lines and entries beyond the kernels' limits."""
    for name in ("hand", "random_a"):
        texts, res = worlds[name]
        a = rule.arrays(*texts)
        text, o = a["text"].decode(), a["t_off"]
        strings = lambda j: tuple(text[int(o[4 * j + k]):int(o[4 * j + k + 1])] for k in range(4))
        for j in range(a["n"]):
            seq, structure = strings(int(res["src"][j]))[:2]
            retyped, at = predict.host_report_line(seq, structure, strings(j)[2], strings(j)[3])
            arm = (int(a["flags"][j]) >> 3) & 3
            assert (retyped and arm != 2) == bool(res["state"][j] & 2) and at == res["stable_idx"][j]
        rt, so = a["row_text"].decode(), a["row_soff"]
        rows = lambda j: [(rt[int(so[r]):int(so[r + 1])], int(a["row_start"][r]), int(a["row_end"][r]), int(a["row_count"][r]))
                          for r in range(int(a["r_off"][j]), int(a["r_off"][j + 1]))]
        for e in range(res["n_entries"]):
            m, p = int(res["ent_m"][e]), int(res["ent_p"][e])
            clusters = [(rows(x), int(res["stable_idx"][x]), len(strings(x)[3]), int(res["pos_adj"][x][0]), int(res["pos_adj"][x][1]),
                         bool(a["flags"][x] & 32)) for x in ((m,) if p < 0 else (m, p))]
            lead, trail, sums, total, ragged = predict.host_report_entry(strings(int(res["src"][m]))[0], clusters)
            r0, r1, p0, p1 = (int(v) for v in (res["row_off"][e], res["row_off"][e + 1], res["prof_off"][e], res["prof_off"][e + 1]))
            assert lead == res["lead"][r0:r1].tolist() and trail == res["trail"][r0:r1].tolist() and sums == res["prof"][p0:p1].tolist()
            assert total == res["total"][e] and int(ragged) == res["flag"][e] & 1


def test_interfaces_name_the_option():
    from mirge_amd import cli
    args = cli.build_parser().parse_args(["annotate", "-s", "x.fastq", "-lib", "lib", "-sp", "human", "-ex", "x", "--novel-report"])
    assert args.novel_report and all(cli.novel_stages(args))
    with pytest.raises(ValueError):
        predict.map_and_cluster(None, "reads.fa", "genome", 3, 25, 14, "out", report=True)
