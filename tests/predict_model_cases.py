"""Inputs for the tests of predict mode's classification: screened-table texts whose rows are de-standardised support vectors
of the fixture model, perturbed with a fixed seed and written in the table's own formats, with rows for every clause of the
filters; hand-made small models; and a writer of the model files' pickle layout (standard library only) for the reader's
tests.  tests/golden/make_predict_model_golden.py runs the reference over the worlds; tests/golden/predict_model.json holds
what it gave."""
import base64
import hashlib
import json
import os
import struct
import zlib

import numpy as np

from mirge_amd.svm_model import SvmModel
from tests import predict_features_model as features_model
from tests import predict_screen_model as screen_model

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "predict_model.json")
TABLE = "unmapped_mirna_smp_vs_representative_seq_modified_selected_sorted_features_updated_stableClusterSeq_15.tsv"
HEADER = (features_model.HEADER_HEAD + features_model.HEADER_TAIL.strip("\n") + "\t" + screen_model.HEADER_TAIL).strip("\n").split("\t")
INT_COLUMNS = {"headUnstableLength", "tailUnstableLength", "distanceToloop", "hairpin_count", "binding_count", "interiorLoopCount",
               "apicalLoop_size", "stem_length", "count_bindings_in_miRNA"}
TWO_DECIMALS = {"percentage_PairedInMiRNA", "mFE"}
NOISE = 0.7
STOP_MARGIN = 1e-6          # relative, around the coupling's eps
WORLDS = (("main", 420, 20261021), ("absent", 60, 7), ("stray", 60, 11))   # name, generated rows, seed


CLIP_HIGH = {"count_bindings_in_miRNA": "20", "exactMatchRatio": "0.4", "mFE": "-39.50", "head_minus3_TemplateNucleotide_percentage": "0.1",
             "hairpin_count": "1", "stem_length": "34", "distanceToloop": "1", "percentage_PairedInMiRNA": "0.75", "headUnstableLength": "0",
             "tail_plus2_A_percentage": "0.5", "head_minus2_TemplateNucleotide_percentage": "0.3", "binding_count": "34",
             "tail_plus1_A_percentage": "0.4", "tail_plus3_A_percentage": "0.4", "tail_plus5_TemplateNucleotide_percentage": "0.3",
             "tail_plus1_TemplateNucleotide_percentage": "0.6", "interiorLoopCount": "5", "head_minus1_TemplateNucleotide_percentage": "0.4",
             "pair_state": "No", "armType": "arm5"}
CLIP_LOW = {"count_bindings_in_miRNA": "7", "exactMatchRatio": "0.0", "mFE": "-38.50", "head_minus3_TemplateNucleotide_percentage": "0.0",
            "hairpin_count": "1", "stem_length": "25", "distanceToloop": "10", "percentage_PairedInMiRNA": "1.00", "headUnstableLength": "3",
            "tail_plus2_A_percentage": "0.0", "head_minus2_TemplateNucleotide_percentage": "0.0", "binding_count": "25",
            "tail_plus1_A_percentage": "0.2", "tail_plus3_A_percentage": "0.0", "tail_plus5_TemplateNucleotide_percentage": "0.0",
            "tail_plus1_TemplateNucleotide_percentage": "0.5", "interiorLoopCount": "6", "head_minus1_TemplateNucleotide_percentage": "0.5",
            "pair_state": "No", "armType": "arm5"}


def golden():
    with open(GOLDEN) as fh:
        return json.load(fh)


def text_digest(text):
    return hashlib.sha256(text.encode("utf-8") if isinstance(text, str) else text).hexdigest()


# ------------------------------------------------------------------------------------------------ the fixture's model
def pack_array(a):
    """float64 bytes, deflated and base64 (a matrix column by column: a feature's values repeat, so it deflates to a fifth)."""
    a = np.asarray(a, dtype="<f8")
    return base64.b64encode(zlib.compress(np.ascontiguousarray(a.T).tobytes(), 9)).decode("ascii")


def unpack_array(text, shape):
    flat = np.frombuffer(zlib.decompress(base64.b64decode(text)), dtype="<f8")
    return np.ascontiguousarray(flat.reshape(shape[::-1]).T)


def model_to_json(m):
    return dict(nf=int(m.sv.shape[1]), n_sv=int(m.sv.shape[0]), mean=pack_array(m.mean), scale=pack_array(m.scale), sv=pack_array(m.sv),
                coef=pack_array(m.coef), intercept=repr(m.intercept), gamma=repr(m.gamma), probA=repr(m.probA), probB=repr(m.probB),
                feature_names=list(m.feature_names))


def model_from_json(d):
    nf, n_sv = d["nf"], d["n_sv"]
    return SvmModel(unpack_array(d["mean"], (nf,)), unpack_array(d["scale"], (nf,)), unpack_array(d["sv"], (n_sv, nf)),
                    unpack_array(d["coef"], (n_sv,)), float(d["intercept"]), float(d["gamma"]), float(d["probA"]), float(d["probB"]),
                    tuple(d["feature_names"]))


_MODEL = []


def fixture_model():
    """The human model's arrays, from the fixture (read once)."""
    if not _MODEL:
        _MODEL.append(model_from_json(golden()["model"]))
    return _MODEL[0]


# ------------------------------------------------------------------------------------------------ table texts
def _default_row(k):
    start = 30 + 200 * k
    row = dict.fromkeys(HEADER, "0")
    row.update(realMicRNA="Null", realMicRNAName="Null", chr="chr1", startPos=str(start), endPos=str(start + 21),
               clusterName="smp:miRCluster_%d_22:chr1:%d_%d+" % (k + 1, start, start + 21), clusterSeq="GTTCTAGTACTGGCCCATTGTA",
               majoritySeq="GTTCTAGTACTGGCCCATTGTA", stableClusterSeq="GTTCTAGTACTGGCCCATTGTA", alignedClusterSeq="GTTCTAGTACTGGCCCATTGTA",
               adjustedClusterSeq="---GTTCTAGTACTGGCCCATTGTA------", clusterSecondSeq="-----TCTAGTACTGGCCCATTG--------",
               templateSeq="GGAGTTCTAGTACTGGCCCATTGTACGTCGC", seqCount=str(3 + k % 5), readCountSum=str(10 + 7 * (k % 9)), exactMatchRatio="1.0",
               neighborState="Good" if k % 3 else "Bad", upstreamDistance="None" if k % 4 == 0 else str(9 + k % 30),
               downstreamDistance=str(9 + k % 35), pruned_precusor_seq="AUUGUACGUCGCAGCAACCCUUGGCGAGCGGAUGCAACGAUCCGCUGGUCGUUUAGC",
               pruned_precusor_str=".........(((...........)))(((((((......)))))))...........", armType="arm5", pair_state="Yes",
               UGU_UGUG_motif="Yes" if k % 2 else "No")
    for name in HEADER:
        if name.endswith("_templateNucleotide"):
            row[name] = "ACGT"[(k + len(name)) % 4]
    return row


def _cell(name, v):
    if name in INT_COLUMNS:
        return str(int(round(v)))
    if name in TWO_DECIMALS:
        return "%.2f" % v
    return features_model.py2_str(float(v))


def _rows(model, n, seed, loops=True, both_states=True, noise=NOISE):
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, model.sv.shape[0], n)
    x = (model.sv[idx] + noise * rng.standard_normal((n, model.sv.shape[1]))) * model.scale + model.mean
    names = list(model.feature_names)
    rows = []
    for k in range(n):
        row = _default_row(k)
        for j, f in enumerate(names):
            if f in row:
                row[f] = _cell(f, x[k, j])
        if "pair_state_Yes" in names and both_states:
            yes = x[k, names.index("pair_state_Yes")]
            no = x[k, names.index("pair_state_No")] if "pair_state_No" in names else 1.0 - yes
            row["pair_state"] = "Yes" if yes > no else "No"
        if "armType_loop" in names:
            loop = loops and x[k, names.index("armType_loop")] > 0.5
            row["armType"] = "loop" if loop else ("arm5", "arm3", "unmatchedRegion")[k % 3]
        rows.append(row)
    return rows


def _none_structure(row):
    for name in screen_model.HEADER_TAIL.strip("\n").split("\t"):
        row[name] = "None"


def world_rows(model, name, n, seed):
    """The rows of a world as dicts, in order, each tagged with the clause it is there for (`_what`)."""
    rows = _rows(model, n, seed, loops=name != "absent", both_states=name != "absent")
    for r in rows:
        r["_what"] = "plain"
    extra = _rows(model, 12, seed + 1, loops=name != "absent", both_states=name != "absent")
    for k, r in enumerate(extra):
        r["clusterName"] = "smp:miRCluster_x%d_22:chr2:%d_%d-" % (k, 50 + k, 71 + k)
    extra[0].update(readCountSum="9", _what="count_below_10")
    extra[1].update(seqCount="2", _what="fewer_than_3_sequences")
    extra[2].update(head_minus1_templateNucleotide="N", _what="cell_equal_N")
    extra[3].update(neighborState="Not", upstreamDistance="None", _what="cell_containing_N")
    _none_structure(extra[4])
    extra[4]["_what"] = "none_structure"
    extra[5].update(readCountSum="10", seqCount="3", _what="counts_at_the_limits")
    extra[6].update(templateSeq="N", _what="N_before_seqCount")
    if name == "main":   # (found by scanning this row's mFE: the decision value at which the coupling stops before its first round)
        extra[6]["mFE"] = "-37.10"
    for r in extra[7:]:
        r["_what"] = "plain"
    if name == "main":   # (found by a coordinate search over formatted cells from the extreme support vectors: decision values
        extra[8].update(CLIP_HIGH, _what="clip_high")   # of +8.2 and -8.5, beyond the +5.25 / -5.1 at which the pairwise
        extra[9].update(CLIP_LOW, _what="clip_low")     # probability is clipped)
    if name == "stray":
        extra[7].update(hairpin_count="many", _what="stray_string")
    # the clause rows go in between the others
    step = max(1, len(rows) // len(extra))
    for k, r in enumerate(extra):
        rows.insert(min(len(rows), k * step + 1), r)
    return rows


def table_text(rows, drop=()):
    drop = set(drop)
    lines = ["\t".join(HEADER)]
    lines += ["\t".join(r[name] for name in HEADER) for k, r in enumerate(rows) if k not in drop]
    return "\n".join(lines) + "\n"


def world_text(model, name, drop=None):
    """The table text of a named world; drop: the row indices left out (None: the fixture's open rows)."""
    n, seed = {w[0]: w[1:] for w in WORLDS}[name]
    if drop is None:
        drop = next(w["dropped"] for w in golden()["worlds"] if w["name"] == name)
    return table_text(world_rows(model, name, n, seed), drop)


def species_text(model, n=80, seed=31, noise=0.25):
    """A plain table close to the support vectors of any of the three models (the maker's check of the reader per model file)."""
    return table_text(_rows(model, n, seed, noise=noise))


def header_only_text():
    return "\t".join(HEADER) + "\n"


def timing_text(model, n_rows, seed=5):
    """A table of about n_rows retained rows (scripts/predict_model_timing.py)."""
    return table_text(_rows(model, n_rows, seed))


# ------------------------------------------------------------------------------------------------ open rows
def prob_margin(model, t):
    return t * max(1.0, abs(model.probA) / 4.0)


def open_rows(model, res, t):
    """The rows of a classify() result that sit closer than a margin to a threshold: the decision value to 0, the printed
    probability to 0.8, two kept probabilities to each other (unless both were clipped to the same value), the coupling's
    stopping quantity to eps at any round."""
    from tests import predict_model_model as rule
    tp = prob_margin(model, t)
    top = res["prob"].max(axis=1)
    out = set()
    for k in range(len(top)):
        if abs(res["dec"][k]) <= t or abs(top[k] - rule.CUTOFF) <= tp:
            out.add(k)
        if any(abs(e - rule.COUPLING_EPS) <= STOP_MARGIN * rule.COUPLING_EPS for e in res["errors"][k]):
            out.add(k)
    kept = sorted((k for k in range(len(top)) if res["pred"][k] == 1 and top[k] >= rule.CUTOFF), key=lambda k: top[k])
    for a, b in zip(kept, kept[1:]):
        if top[b] - top[a] <= tp and not (res["clipped"][a] and res["clipped"][b]):
            out.update((a, b))
    return out


# ------------------------------------------------------------------------------------------------ hand-made models
def hand_model(nf, n_sv, seed=0, gamma=0.1, coef_scale=10.0, spread=1.0, prob_a=-2.0, prob_b=0.1):
    """A small model of random arrays: support vectors of `spread` around 0, coefficients of both signs up to coef_scale (the
    real models' are bounded by C = 10); a single support vector has the coefficient coef_scale itself."""
    rng = np.random.default_rng(1000 * nf + n_sv + seed)
    sv = spread * rng.standard_normal((n_sv, nf))
    coef = coef_scale * rng.uniform(-1.0, 1.0, n_sv)
    if n_sv == 1:
        coef[0] = coef_scale
    mean, scale = rng.uniform(-2.0, 2.0, nf), rng.uniform(0.5, 3.0, nf)
    return SvmModel(mean, scale, sv, coef, float(rng.uniform(-0.5, 0.5)), float(gamma), float(prob_a), float(prob_b),
                    tuple("f%d" % j for j in range(nf)))


def hand_rows(model, n, seed=0, noise=0.5):
    rng = np.random.default_rng(seed + 17)
    idx = rng.integers(0, model.sv.shape[0], n)
    return (model.sv[idx] + noise * rng.standard_normal((n, model.sv.shape[1]))) * model.scale + model.mean


# ------------------------------------------------------------------------------------------------ a writer of the pickle layout
class PickleWriter:
    """Protocol-2 opcodes of joblib's old layout by hand: objects by GLOBAL / EMPTY_TUPLE / NEWOBJ / state / BUILD, an array
    as a NumpyArrayWrapper whose bytes follow its BUILD."""

    def __init__(self):
        self.out = [b"\x80\x02"]

    def raw(self, b):
        self.out.append(b)

    def glob(self, module, name):
        self.raw(b"c" + module.encode() + b"\n" + name.encode() + b"\n")

    def string(self, s):
        b = s.encode("latin1")
        self.raw(b"U" + bytes([len(b)]) + b if len(b) < 256 else b"T" + struct.pack("<i", len(b)) + b)

    def integer(self, v):
        self.raw(b"J" + struct.pack("<i", v))

    def floating(self, v):
        self.raw(b"G" + struct.pack(">d", v))

    def boolean(self, v):
        self.raw(b"\x88" if v else b"\x89")

    def none(self):
        self.raw(b"N")

    def value(self, v):
        if isinstance(v, Fortran):
            self.array(v.a, "F")
        elif isinstance(v, Inline):
            self.inline_array(v.a)
        elif isinstance(v, np.generic):
            self.scalar(v)
        elif isinstance(v, np.ndarray):
            self.array(v)
        elif isinstance(v, bool):
            self.boolean(v)
        elif isinstance(v, int):
            self.integer(v)
        elif isinstance(v, float):
            self.floating(v)
        elif isinstance(v, str):
            self.string(v)
        elif v is None:
            self.none()
        elif isinstance(v, tuple):
            self.raw(b"(")
            for x in v:
                self.value(x)
            self.raw(b"t")
        elif isinstance(v, list):
            self.raw(b"](")
            for x in v:
                self.value(x)
            self.raw(b"e")
        elif isinstance(v, Obj):
            self.obj(v)
        else:
            raise TypeError(type(v))

    def obj(self, o):
        self.glob(o.module, o.name)
        if not o.state:   # (NEWOBJ alone: no BUILD)
            self.raw(b")\x81")
            return
        self.raw(b")\x81}(")
        for k, v in o.state.items():
            self.string(k)
            self.value(v)
        self.raw(b"ub")

    def dtype(self, code):
        self.glob("numpy", "dtype")
        self.string(code)
        self.raw(b"K\x00K\x01\x87R(K\x03")
        self.string("<" if code not in ("i1", "u1", "b1") else "|")
        self.raw(b"NNNJ\xff\xff\xff\xffJ\xff\xff\xff\xffK\x00tb")

    def array(self, a, order="C"):
        self.glob("sklearn.externals.joblib.numpy_pickle", "NumpyArrayWrapper")
        self.raw(b")\x81}(")
        self.string("dtype")
        self.dtype(a.dtype.str[1:])
        self.string("shape")
        self.value(tuple(int(d) for d in a.shape))
        self.string("order")
        self.string(order)
        self.string("subclass")
        self.glob("numpy", "ndarray")
        self.string("allow_mmap")
        self.boolean(True)
        self.raw(b"ub")
        self.raw(np.asarray(a).tobytes(order=order))

    def inline_array(self, a):
        """numpy's own pickle of an array: _reconstruct(ndarray, (0,), 'b') and the state (1, shape, dtype, False, bytes)."""
        self.glob("numpy.core.multiarray", "_reconstruct")
        self.raw(b"(")
        self.glob("numpy", "ndarray")
        self.raw(b"K\x00\x85")
        self.string("b")
        self.raw(b"tR(K\x01")
        self.value(tuple(int(d) for d in a.shape))
        self.dtype(a.dtype.str[1:])
        self.boolean(False)
        self.string(a.tobytes().decode("latin1"))
        self.raw(b"tb")

    def scalar(self, v):
        self.glob("numpy.core.multiarray", "scalar")
        self.raw(b"(")
        self.dtype(v.dtype.str[1:])
        self.string(v.tobytes().decode("latin1"))
        self.raw(b"tR")

    def done(self):
        return zlib.compress(b"".join(self.out) + b".")


class Obj:
    def __init__(self, module, name, **state):
        self.module, self.name, self.state = module, name, state


class Fortran:
    """An array to be written in Fortran order (joblib then stores the bytes of its transpose)."""

    def __init__(self, a):
        self.a = a


class Inline:
    """An array to be written as numpy pickles one, not behind a NumpyArrayWrapper."""

    def __init__(self, a):
        self.a = a


def model_file_bytes(m, kernel="rbf", classes=(-1, 1), coef_shape=None, extra_global=None, probability=True, sparse=False,
                     with_mean=True, steps=1, sv_order="C", inline=False, state=True):
    """The bytes of a model file holding m, or one of the variations: sv_order "F" (the support vectors in Fortran order),
    inline (intercept_ as numpy's own pickle, _gamma as a numpy scalar), state=False (an SVC that is never given its state)
    and the ones the reader refuses."""
    w = PickleWriter()
    n_sv, nf = m.sv.shape
    scaler = Obj("sklearn.preprocessing.data", "StandardScaler", mean_=m.mean, scale_=m.scale, var_=m.scale ** 2, with_mean=with_mean,
                 with_std=True, copy=True, n_samples_seen_=100)
    coef = m.coef.reshape(coef_shape if coef_shape else (1, n_sv))
    svc_state = dict(kernel=kernel, gamma=m.gamma, _gamma=m.gamma, probability=probability, _sparse=sparse,
                     classes_=np.array(classes, dtype="<i8"), support_vectors_=m.sv, dual_coef_=coef, intercept_=np.array([m.intercept]),
                     probA_=np.array([m.probA]), probB_=np.array([m.probB]), C=1.0)
    if extra_global:
        svc_state["hook"] = Obj(*extra_global)
    if sv_order == "F":
        svc_state["support_vectors_"] = Fortran(m.sv)
    if inline:
        svc_state.update(intercept_=Inline(np.array([m.intercept])), _gamma=np.float64(m.gamma))
    svc = Obj("sklearn.svm.classes", "SVC", **(svc_state if state else {}))
    pipe = Obj("sklearn.pipeline", "Pipeline", steps=[("clf", svc)] * steps)
    w.raw(b"](")
    w.obj(scaler)
    w.obj(pipe)
    w.value([(1.0 - 0.01 * j, j, f) for j, f in enumerate(m.feature_names)])
    w.raw(b"e")
    return w.done()


def write_model_dir(path, m, species="human", namelist=None, **variation):
    os.makedirs(path, exist_ok=True)
    with open(os.path.join(path, "%s_svc_model.pkl" % species), "wb") as fh:
        fh.write(model_file_bytes(m, **variation))
    with open(os.path.join(path, "total_features_namelist.txt"), "w") as fh:
        fh.write("\n".join(namelist if namelist is not None else golden()["namelist"]) + "\n")
    return path
