"""The reader of miRge2.0's SVM model files (`models/<species>_svc_model.pkl`, `models/total_features_namelist.txt`) for
predict mode's classification.  Standard library and numpy only: neither sklearn nor joblib is imported.

A model file is a zlib stream holding a protocol-2 pickle in joblib's old layout (sklearn 0.18.1): the list
[StandardScaler, Pipeline([('clf', SVC)]), [(score, index, feature name), ...]], every array a NumpyArrayWrapper object
whose bytes follow its BUILD opcode in the stream.  The pickle is read by a subclass of the pure-Python unpickler whose
find_class resolves the names of ALLOWED alone, each to an inert holder (a class that keeps the state it is given and runs
nothing): any other global is an error naming it.  That is why a user's pickle may be opened at all.

    model = load_model(model_dir, "human")     # SvmModel: mean, scale, sv, coef, intercept, gamma, probA, probB, feature_names
    names = read_namelist(model_dir)           # total_features_namelist.txt, first occurrences in order
"""
import io
import os
import pickle
import zlib
from collections import namedtuple

import numpy as np

MAX_FEATURES = 64      # the kernel keeps a row's features in registers (csrc/predict_svm.hpp: kSvmMaxFeatures)
MAX_PICKLE_BYTES = 1 << 30   # what a model file may inflate to (the three real ones: 0.2 to 0.35 MB), and an array hold
NAMELIST = "total_features_namelist.txt"

SvmModel = namedtuple("SvmModel", "mean scale sv coef intercept gamma probA probB feature_names")


class ModelError(ValueError):
    """A model file this engine refuses; the message names the file and the field."""


class _Holder:
    """What an allowed class name resolves to: it keeps the state a BUILD gives it and does nothing else."""

    args, state = (), None      # (NEWOBJ makes an object without __init__; a damaged pickle may never BUILD it)

    def __init__(self, *args):
        self.args = args
        self.state = None

    def __setstate__(self, state):
        self.state = state

    def get(self, key, what):
        if not isinstance(self.state, dict) or key not in self.state:
            raise ModelError("%s: no field %s" % (what, key))
        return self.state[key]


class _Scaler(_Holder):
    pass


class _Pipeline(_Holder):
    pass


class _Svc(_Holder):
    pass


class _ArrayWrapper(_Holder):
    pass


class _Ndarray(_Holder):
    """A numpy.ndarray pickled the ordinary way (numpy.core.multiarray._reconstruct and a state tuple)."""

    def array(self):
        try:
            _version, shape, dtype, fortran, data = self.state
            if isinstance(data, str):
                data = data.encode("latin1")
            a = np.frombuffer(data, dtype=dtype.numpy()).copy()
            return a.reshape(shape, order="F" if fortran else "C")
        except ModelError:
            raise
        except Exception as e:
            raise ModelError("an inline array cannot be rebuilt: %s" % e)


class _Dtype(_Holder):
    _PLAIN = ("f8", "f4", "i8", "i4", "i2", "i1", "u8", "u4", "u2", "u1", "b1")

    def numpy(self):
        code = self.args[0] if self.args else None
        if code not in self._PLAIN:
            raise ModelError("an array of dtype %r: only plain numeric arrays are read" % (code,))
        order = self.state[1] if isinstance(self.state, tuple) and len(self.state) > 1 else "|"
        if order not in ("<", "|", "="):
            raise ModelError("an array of byte order %r" % (order,))
        return np.dtype(("<" if order != "|" else "|") + code)


def _reconstruct(cls, shape, code):
    if cls is not _Ndarray:
        raise ModelError("_reconstruct of %r" % (cls,))
    return _Ndarray()


def _scalar(dtype, data):
    if isinstance(data, str):
        data = data.encode("latin1")
    return np.frombuffer(data, dtype=dtype.numpy())[0]


# every global a model file may name
ALLOWED = {
    ("sklearn.preprocessing.data", "StandardScaler"): _Scaler,
    ("sklearn.preprocessing._data", "StandardScaler"): _Scaler,
    ("sklearn.pipeline", "Pipeline"): _Pipeline,
    ("sklearn.svm.classes", "SVC"): _Svc,
    ("sklearn.svm._classes", "SVC"): _Svc,
    ("sklearn.externals.joblib.numpy_pickle", "NumpyArrayWrapper"): _ArrayWrapper,
    ("joblib.numpy_pickle", "NumpyArrayWrapper"): _ArrayWrapper,
    ("numpy", "dtype"): _Dtype,
    ("numpy", "ndarray"): _Ndarray,
    ("numpy.core.multiarray", "_reconstruct"): _reconstruct,
    ("numpy.core.multiarray", "scalar"): _scalar,
}


class _Unpickler(pickle._Unpickler):
    """The pure-Python unpickler (its opcode table can be extended), with the allowlist and joblib's inline arrays."""

    dispatch = dict(pickle._Unpickler.dispatch)

    def __init__(self, stream):
        super().__init__(stream, encoding="latin1")
        self._stream = stream

    def find_class(self, module, name):
        try:
            return ALLOWED[(module, name)]
        except KeyError:
            raise ModelError("the pickle names the global %s.%s, which a model file has no use for" % (module, name))

    def get_extension(self, code):
        raise ModelError("the pickle names an extension code, which a model file has no use for")

    def persistent_load(self, pid):
        raise ModelError("the pickle names a persistent object, which a model file has no use for")

    def load_build(self):
        super().load_build()
        top = self.stack[-1]
        if isinstance(top, _ArrayWrapper):
            self.stack[-1] = self._inline_array(top)

    dispatch[pickle.BUILD[0]] = load_build

    def _inline_array(self, w):
        what = "an inline array"
        shape, order, dtype = w.get("shape", what), w.get("order", what), w.get("dtype", what)
        if not isinstance(dtype, _Dtype) or not isinstance(shape, tuple) or not all(isinstance(d, int) and d >= 0 for d in shape):
            raise ModelError("%s: shape %r, dtype %r" % (what, shape, dtype))
        dt = dtype.numpy()
        count = 1
        for d in shape:
            count *= d
        if count * dt.itemsize > MAX_PICKLE_BYTES:
            raise ModelError("%s of shape %r: more than 1 GiB" % (what, shape))
        raw = self._stream.read(count * dt.itemsize)
        if len(raw) != count * dt.itemsize:
            raise ModelError("%s of shape %r: the stream ends inside it" % (what, shape))
        a = np.frombuffer(raw, dtype=dt).copy()
        if order == "F":
            return a.reshape(shape[::-1]).transpose()
        return a.reshape(shape)


def _array(x, what):
    if isinstance(x, _Ndarray):
        x = x.array()
    if not isinstance(x, np.ndarray):
        raise ModelError("%s is no array" % what)
    return x


def _text(x):
    return x.decode("latin1") if isinstance(x, bytes) else x


def parse_model(raw, what="model"):
    """SvmModel from the bytes of a model file.  ModelError (a ValueError) names `what` and the field it refuses."""
    try:
        inflate = zlib.decompressobj()
        data = inflate.decompress(raw, MAX_PICKLE_BYTES + 1)
    except zlib.error as e:
        raise ModelError("%s: no zlib stream (%s)" % (what, e))
    if len(data) > MAX_PICKLE_BYTES:
        raise ModelError("%s: the pickle is larger than %d bytes" % (what, MAX_PICKLE_BYTES))
    try:
        obj = _Unpickler(io.BytesIO(data)).load()
    except ModelError as e:
        raise ModelError("%s: %s" % (what, e))
    except Exception as e:   # a damaged stream: whatever the opcode at hand raises
        raise ModelError("%s: the pickle cannot be read (%s: %s)" % (what, type(e).__name__, e))
    try:
        return _checked(obj)
    except ModelError as e:
        raise ModelError("%s: %s" % (what, e))
    except Exception as e:   # a field of a kind no check expects
        raise ModelError("%s: contents that cannot be read (%s: %s)" % (what, type(e).__name__, e))


def _checked(obj):
    if not isinstance(obj, list) or len(obj) != 3:
        raise ModelError("contents: expected the list [scaler, pipeline, selected features]")
    sc, pipe, selected = obj
    if not isinstance(sc, _Scaler):
        raise ModelError("contents: the first item is no StandardScaler")
    if not isinstance(pipe, _Pipeline):
        raise ModelError("contents: the second item is no Pipeline")
    for flag in ("with_mean", "with_std"):
        if sc.get(flag, "scaler") is not True:
            raise ModelError("scaler: %s is off" % flag)
    f64 = lambda x, name: np.ascontiguousarray(_array(x, name), dtype=np.float64)
    mean, scale = f64(sc.get("mean_", "scaler"), "scaler: mean_"), f64(sc.get("scale_", "scaler"), "scaler: scale_")
    steps = pipe.get("steps", "pipeline")
    if not isinstance(steps, list) or len(steps) != 1:
        raise ModelError("pipeline: steps: expected one step, found %s" % (len(steps) if isinstance(steps, list) else "no list"))
    if not isinstance(steps[0], tuple) or len(steps[0]) != 2 or not isinstance(steps[0][1], _Svc):
        raise ModelError("pipeline: steps: the step is no SVC")
    svc = steps[0][1]
    kernel = _text(svc.get("kernel", "SVC"))
    if kernel != "rbf":
        raise ModelError("SVC: kernel is %r, not 'rbf'" % (kernel,))
    if svc.get("probability", "SVC") is not True:
        raise ModelError("SVC: probability is off")
    if svc.get("_sparse", "SVC") is not False:
        raise ModelError("SVC: _sparse is set: the model was fitted on sparse data")
    classes = _array(svc.get("classes_", "SVC"), "SVC: classes_")
    if classes.shape != (2,) or int(classes[0]) != -1 or int(classes[1]) != 1:
        raise ModelError("SVC: classes_ is %s, not [-1, 1]" % (classes.tolist(),))
    sv = f64(svc.get("support_vectors_", "SVC"), "SVC: support_vectors_")
    coef = f64(svc.get("dual_coef_", "SVC"), "SVC: dual_coef_")
    intercept = f64(svc.get("intercept_", "SVC"), "SVC: intercept_")
    prob_a, prob_b = f64(svc.get("probA_", "SVC"), "SVC: probA_"), f64(svc.get("probB_", "SVC"), "SVC: probB_")
    gamma = float(svc.get("_gamma", "SVC"))
    if sv.ndim != 2 or sv.shape[0] < 1:
        raise ModelError("SVC: support_vectors_ has shape %s" % (sv.shape,))
    n_sv, nf = sv.shape
    if nf < 1 or nf > MAX_FEATURES:
        raise ModelError("SVC: support_vectors_ has %d features; this engine takes 1 to %d" % (nf, MAX_FEATURES))
    if coef.shape != (1, n_sv):
        raise ModelError("SVC: dual_coef_ has shape %s for %d support vectors" % (coef.shape, n_sv))
    for name, a in (("intercept_", intercept), ("probA_", prob_a), ("probB_", prob_b)):
        if a.shape != (1,):
            raise ModelError("SVC: %s has shape %s, not (1,)" % (name, a.shape))
    if mean.shape != (nf,) or scale.shape != (nf,):
        raise ModelError("scaler: mean_ %s and scale_ %s for %d features" % (mean.shape, scale.shape, nf))
    if not (gamma > 0.0) or not np.isfinite(gamma):
        raise ModelError("SVC: _gamma is %r" % (gamma,))
    for name, a in (("mean_", mean), ("scale_", scale), ("support_vectors_", sv), ("dual_coef_", coef), ("intercept_", intercept),
                    ("probA_", prob_a), ("probB_", prob_b)):
        if not np.isfinite(a).all():
            raise ModelError("%s holds a value that is not finite" % name)
    if (scale == 0.0).any():
        raise ModelError("scaler: scale_ holds a zero")
    if not isinstance(selected, list) or len(selected) != nf:
        raise ModelError("selected features: %s names for %d features" % (len(selected) if isinstance(selected, list) else "no list of", nf))
    names = []
    for item in selected:
        if not isinstance(item, tuple) or len(item) != 3 or not isinstance(item[2], (str, bytes)):
            raise ModelError("selected features: an item that is no (score, index, name)")
        names.append(_text(item[2]))
    return SvmModel(mean, scale, sv, np.ascontiguousarray(coef[0]), float(intercept[0]), gamma, float(prob_a[0]), float(prob_b[0]), tuple(names))


def model_path(model_dir, species):
    """The reference's choice (miRge2.0.py:636-641): human and mouse have a model of their own, every other species `others`."""
    return os.path.join(model_dir, "%s_svc_model.pkl" % (species if species in ("human", "mouse") else "others"))


def load_model(model_dir, species):
    """SvmModel of `species` from the directory `model_dir`.  OSError where the file cannot be read, ModelError where it is refused."""
    path = model_path(model_dir, species)
    with open(path, "rb") as f:
        raw = f.read()
    return parse_model(raw, path)


def read_namelist(model_dir):
    """The names of total_features_namelist.txt as preprocess_featureFiles takes them: stripped lines, first occurrences."""
    path = os.path.join(model_dir, NAMELIST)
    names = []
    with open(path, "r") as f:
        for line in f:
            if line.strip() not in names:
                names.append(line.strip())
    if not any(names):
        raise ModelError("%s: no names" % path)
    return names
