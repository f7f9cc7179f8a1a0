"""The accent-drift classifier as plain tables: random-forest inference on the GPU (the classifier half).

The reference scores a segment's 286-d feature vector with a pickled scikit-learn model (validation/classifier/trainer.py:217-227,
validation/classifier/__init__.py:115-118): ``CalibratedClassifierCV(RandomForestClassifier(n_estimators=200, max_depth=10, ...),
method='isotonic', cv=5)`` - five forests of 200 trees with one isotonic calibrator each, ``predict_proba(x)[0][1]`` averaged over
the five.  This package never unpickles: ``tools/export_drift_classifier.py`` turns the pickle into the arrays below once
(``export_sklearn``), and everything here - ``validate``, ``predict_host``, ``DriftForest`` - works on those arrays alone.

The table format, version 1 (a dict of numpy arrays; ``save`` / ``load`` keep it as an ``.npz`` read with ``allow_pickle=False``):

  scalars      ``version`` int32 = 1, ``n_features`` int32, ``optimal_threshold`` float64 (the trainer's metadata, 0.18 when absent)
  forests      ``forest_first`` int32 [n_forests + 1]: forest c owns the trees forest_first[c] .. forest_first[c + 1] - 1
  nodes        ``tree_first`` int32 [n_trees + 1]: tree t owns the nodes tree_first[t] .. tree_first[t + 1] - 1, its root first;
               per node k (indices count through the whole file):
               ``node_feature`` int32: the split feature, -1 for a leaf;
               ``node_value`` float64: the threshold of a split node / the class-1 fraction of a leaf, exactly what that
               scikit-learn version's ``DecisionTreeClassifier.predict_proba`` returns for it;
               ``node_right`` int32: the right child of a split node (-1 for a leaf).  The LEFT child is always k + 1: scikit-learn
               stores a tree in depth-first pre-order, and the exporter verifies that before it drops the column.  On the device
               a node is 16 bytes (value, feature, right child): one load per level.
  calibrators  ``iso_first`` int32 [n_calibrators + 1], ``iso_x`` / ``iso_y`` float64: the knots (``X_thresholds_`` /
               ``y_thresholds_``) of calibrator c = forest c's.  n_calibrators is n_forests, or 0 for a bare forest (one forest,
               identity calibration).

``predict_host`` is the definition of the two kernels of csrc/forest.hip (as ``features.viterbi_banded`` is of k_feat_viterbi): the
device result equals it bit for bit, row by row, whatever else shares the call.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Union

import numpy as np

from . import _native

FORMAT_VERSION = 1
DEFAULT_OPTIMAL_THRESHOLD = 0.18                   # validation/classifier/__init__.py:18
MAX_DEPTH = 64                                     # edges from a root to its deepest leaf
MAX_FORESTS = 64                                   # one lane of the finishing wave per forest
HANDCRAFTED = 30                                   # features.HandcraftedFeatures' width

_INT_KEYS = ("forest_first", "tree_first", "node_feature", "node_right", "iso_first")
_F64_KEYS = ("node_value", "iso_x", "iso_y")
_SCALARS = (("version", np.int32), ("n_features", np.int32), ("optimal_threshold", np.float64))
KEYS = tuple(k for k, _ in _SCALARS) + _INT_KEYS + _F64_KEYS


# ------------------------------------------------------------------------------------------------ the exporter (host only)
def _refuse(why: str):
    raise ValueError(f"export_sklearn: {why}")


def _export_forest(rf, trees: list) -> None:
    from sklearn.ensemble import RandomForestClassifier
    if not isinstance(rf, RandomForestClassifier):
        _refuse(f"the estimator is a {type(rf).__name__}, not a RandomForestClassifier")
    if int(rf.n_outputs_) != 1:
        _refuse(f"n_outputs is {rf.n_outputs_}, not 1")
    if list(np.asarray(rf.classes_).tolist()) != [0, 1]:
        _refuse(f"the classes are {np.asarray(rf.classes_).tolist()}, not [0, 1]")
    for est in rf.estimators_:
        t = est.tree_
        left, right = np.asarray(t.children_left, dtype=np.int64), np.asarray(t.children_right, dtype=np.int64)
        split = left != -1
        k = np.arange(left.shape[0])
        if not np.array_equal(left[split], k[split] + 1):
            _refuse("a tree is not stored in depth-first pre-order (left child != node + 1)")
        # Without missing values at fit time scikit-learn sends a missing value to the larger child; any other direction was
        # learned from missing values, and such a tree accepts NaN inputs this inference refuses.
        ns = np.asarray(t.n_node_samples, dtype=np.int64)
        go_left = np.asarray(t.missing_go_to_left, dtype=bool)[split]
        if not np.array_equal(go_left, ns[left[split]] > ns[right[split]]):
            _refuse("the trees were trained with missing-value support (NaN features)")
        value = np.asarray(t.value, dtype=np.float64)
        if value.shape[1:] != (1, 2):
            _refuse(f"a tree's value array has shape {value.shape}, not [nodes][1][2]")
        trees.append({"feature": np.where(split, np.asarray(t.feature, dtype=np.int64), -1), "right": np.where(split, right, -1),
                      "value": np.where(split, np.asarray(t.threshold, dtype=np.float64), value[:, 0, 1])})


def export_sklearn(model_or_metadata) -> dict:
    """The tables of a fitted scikit-learn drift classifier: a ``CalibratedClassifierCV`` over ``RandomForestClassifier`` with
    isotonic calibration, the reference's metadata dict around one (``{'model': ..., 'optimal_threshold': ...}``), or a bare
    ``RandomForestClassifier`` (no calibrators).  Anything else is refused with a ``ValueError`` that names the reason."""
    from sklearn.calibration import CalibratedClassifierCV
    from sklearn.ensemble import RandomForestClassifier
    from sklearn.isotonic import IsotonicRegression
    model, threshold = model_or_metadata, DEFAULT_OPTIMAL_THRESHOLD
    if isinstance(model, dict):
        if "model" not in model:
            _refuse("the metadata dict has no 'model'")
        threshold = float(model.get("optimal_threshold", DEFAULT_OPTIMAL_THRESHOLD))
        model = model["model"]
    forests, iso = [], []
    if isinstance(model, CalibratedClassifierCV):
        for cc in model.calibrated_classifiers_:
            if getattr(cc, "method", None) != "isotonic":
                _refuse(f"the calibration is '{getattr(cc, 'method', None)}', not isotonic")
            trees: list = []
            _export_forest(cc.estimator, trees)
            if len(cc.calibrators) != 1 or not isinstance(cc.calibrators[0], IsotonicRegression):
                _refuse("a calibrated classifier does not hold exactly one isotonic calibrator")
            cal = cc.calibrators[0]
            if getattr(cal, "out_of_bounds", None) != "clip":
                _refuse("an isotonic calibrator does not clip out-of-range inputs")
            forests.append(trees)
            iso.append((np.asarray(cal.X_thresholds_, dtype=np.float64), np.asarray(cal.y_thresholds_, dtype=np.float64)))
        n_features = int(model.n_features_in_)
    elif isinstance(model, RandomForestClassifier):
        trees = []
        _export_forest(model, trees)
        forests.append(trees)
        n_features = int(model.n_features_in_)
    else:
        _refuse(f"the estimator is a {type(model).__name__}, not a CalibratedClassifierCV or a RandomForestClassifier")
    forest_first, tree_first, feat, right, value = [0], [0], [], [], []
    for trees in forests:
        for t in trees:
            base = tree_first[-1]
            feat.append(t["feature"])
            right.append(np.where(t["right"] >= 0, t["right"] + base, -1))
            value.append(t["value"])
            tree_first.append(base + t["feature"].shape[0])
        forest_first.append(len(tree_first) - 1)
    iso_first = [0]
    for x, _ in iso:
        iso_first.append(iso_first[-1] + x.shape[0])
    tables = {
        "version": np.int32(FORMAT_VERSION), "n_features": np.int32(n_features), "optimal_threshold": np.float64(threshold),
        "forest_first": np.asarray(forest_first, dtype=np.int32), "tree_first": np.asarray(tree_first, dtype=np.int32),
        "node_feature": np.concatenate(feat).astype(np.int32), "node_right": np.concatenate(right).astype(np.int32),
        "node_value": np.concatenate(value).astype(np.float64), "iso_first": np.asarray(iso_first, dtype=np.int32),
        "iso_x": np.concatenate([x for x, _ in iso]) if iso else np.zeros(0), "iso_y": np.concatenate([y for _, y in iso]) if iso else np.zeros(0)}
    return validate(tables)


# ------------------------------------------------------------------------------------------------ the format
def _bad(why: str):
    raise ValueError(f"drift classifier tables: {why}")


def _ranges(name: str, first: np.ndarray, total: int, what: str) -> None:
    if first.ndim != 1 or first.shape[0] < 1 or int(first[0]) != 0 or int(first[-1]) != total:
        _bad(f"{name} does not cover the {total} {what} contiguously from 0")
    if np.any(np.diff(first) <= 0):
        _bad(f"{name} holds an empty or descending range")


def tree_depth(tables: dict) -> int:
    """Edges from a root to the deepest node a walk can reach (children lie behind their parents, so every walk ends).  More than
    MAX_DEPTH is reported as MAX_DEPTH + 1."""
    feat, right = tables["node_feature"], tables["node_right"].astype(np.int64)
    front = np.unique(tables["tree_first"][:-1].astype(np.int64))
    depth = 0
    while True:
        front = front[feat[front] >= 0]
        if front.size == 0 or depth > MAX_DEPTH:
            return depth
        front = np.unique(np.concatenate([front + 1, right[front]]))
        depth += 1


def validate(tables: dict) -> dict:
    """The tables, normalised (dtypes, C order), or a ``ValueError`` that names what is wrong.  Called by ``load`` and before every
    upload: it is what keeps a bad file from sending a kernel out of bounds or around a cycle.  Every child index lies behind its
    parent and inside its own tree, so every walk terminates and its depth is known here."""
    missing = [k for k in KEYS if k not in tables]
    if missing:
        _bad(f"missing {', '.join(missing)}")
    t = {}
    for k, dt in _SCALARS:
        a = np.asarray(tables[k])
        if a.size != 1 or a.dtype == object:
            _bad(f"{k} is not a scalar")
        t[k] = dt(a.reshape(()))
    for k in _INT_KEYS:
        a = np.asarray(tables[k])
        if a.ndim != 1 or a.dtype.kind not in "iu":
            _bad(f"{k} is not a one-dimensional integer array")
        if a.size and (int(a.min()) < -1 or int(a.max()) > np.iinfo(np.int32).max):
            _bad(f"{k} does not fit int32")
        t[k] = np.ascontiguousarray(a, dtype=np.int32)
    for k in _F64_KEYS:
        a = np.asarray(tables[k])
        if a.ndim != 1 or a.dtype.kind != "f":
            _bad(f"{k} is not a one-dimensional float array")
        t[k] = np.ascontiguousarray(a, dtype=np.float64)
    if int(t["version"]) != FORMAT_VERSION:
        _bad(f"format version {int(t['version'])}, this build reads {FORMAT_VERSION}")
    nf = int(t["n_features"])
    if nf < 1:
        _bad(f"n_features is {nf}")
    if not np.isfinite(t["optimal_threshold"]):
        _bad("optimal_threshold is not finite")
    feat, right, value = t["node_feature"], t["node_right"], t["node_value"]
    n_nodes, n_trees, n_forests = feat.shape[0], t["tree_first"].shape[0] - 1, t["forest_first"].shape[0] - 1
    if right.shape[0] != n_nodes or value.shape[0] != n_nodes:
        _bad("node_feature, node_right and node_value differ in length")
    _ranges("tree_first", t["tree_first"], n_nodes, "nodes")
    _ranges("forest_first", t["forest_first"], n_trees, "trees")
    if n_forests < 1 or n_forests > MAX_FORESTS:
        _bad(f"{n_forests} forests (1 .. {MAX_FORESTS})")
    if np.any(feat < -1) or np.any(feat >= nf):
        _bad(f"a split feature is not below n_features = {nf}")
    if not np.all(np.isfinite(value)):
        _bad("a threshold or leaf value is not finite")
    leaf = feat < 0
    if np.any(value[leaf] < 0.0) or np.any(value[leaf] > 1.0):
        _bad("a leaf value is outside [0, 1]")
    if np.any(right[leaf] != -1):
        _bad("a leaf has a child")
    k = np.arange(n_nodes, dtype=np.int64)
    end = np.repeat(t["tree_first"][1:].astype(np.int64), np.diff(t["tree_first"]))          # one past the last node of k's tree
    split = ~leaf
    if np.any(right[split] <= k[split]):
        _bad("a child index is not greater than its parent's")
    if np.any(right[split] >= end[split]):
        _bad("a child index is outside its tree")
    depth = tree_depth(t)
    if depth > MAX_DEPTH:
        _bad(f"a tree is deeper than {MAX_DEPTH}")
    n_cal = t["iso_first"].shape[0] - 1
    x, y = t["iso_x"], t["iso_y"]
    if x.shape != y.shape:
        _bad("iso_x and iso_y differ in length")
    if n_cal < 0 or int(t["iso_first"][0]) != 0 or int(t["iso_first"][-1]) != x.shape[0]:
        _bad("iso_first does not cover the knots contiguously from 0")
    if np.any(np.diff(t["iso_first"]) <= 0):
        _bad("an empty calibrator (every calibrator needs at least one knot)")
    if n_cal not in (0, n_forests) or (n_cal == 0 and n_forests != 1):
        _bad(f"{n_cal} calibrators for {n_forests} forests (one each, or none for a single forest)")
    if not (np.all(np.isfinite(x)) and np.all(np.isfinite(y))):
        _bad("a calibrator knot is not finite")
    inner = np.ones(max(x.shape[0] - 1, 0), dtype=bool)
    inner[t["iso_first"][1:-1].astype(np.int64) - 1] = False                                   # pairs that straddle two calibrators
    if np.any(np.diff(x)[inner] <= 0):
        _bad("iso_x is not strictly increasing")
    return t


def save(path: str, tables: dict) -> None:
    """Write the tables as a compressed ``.npz`` (plain arrays, nothing pickled)."""
    t = validate(tables)
    with open(path, "wb") as f:
        np.savez_compressed(f, **{k: t[k] for k in KEYS})


def load(path: str) -> dict:
    """Read and validate a file written by ``save``.  Read with ``allow_pickle=False``: a file that needs unpickling is refused."""
    with np.load(path, allow_pickle=False) as z:
        missing = [k for k in KEYS if k not in z.files]
        if missing:
            _bad(f"{path}: missing {', '.join(missing)}")
        return validate({k: z[k] for k in KEYS})


# ------------------------------------------------------------------------------------------------ the definition
def _as_rows(tables: dict, X) -> np.ndarray:
    X = np.asarray(X, dtype=np.float64)
    nf = int(tables["n_features"])
    if X.ndim == 1 and X.shape[0] == nf:
        X = X[None, :]
    if X.ndim != 2 or X.shape[1] != nf:
        raise ValueError(f"the classifier takes [n][{nf}] features, got an array of shape {X.shape}")
    return np.ascontiguousarray(X)


def _to_float32(X: np.ndarray) -> np.ndarray:
    with np.errstate(over="ignore", invalid="ignore"):
        x32 = X.astype(np.float32)
    if not np.all(np.isfinite(x32)):
        raise ValueError("a feature is NaN, infinite or beyond float32's range")
    return x32


def calibrate_host(x: np.ndarray, kx: np.ndarray, ky: np.ndarray) -> np.ndarray:
    """One isotonic calibrator on a vector of forest means: clip to the knots, then ``np.interp``'s own arithmetic, one rounding
    per operation (slope = dy / dx; slope * (x - x_j) + y_j; a value on a knot takes the knot's y; a single knot is a constant)."""
    if kx.shape[0] == 1:
        return np.full(x.shape, ky[0])
    x = np.minimum(np.maximum(x, kx[0]), kx[-1])
    j = np.searchsorted(kx, x, side="right") - 1                                   # kx[j] <= x < kx[j + 1]
    last = j >= kx.shape[0] - 1
    j0 = np.where(last, kx.shape[0] - 2, j)
    slope = (ky[j0 + 1] - ky[j0]) / (kx[j0 + 1] - kx[j0])
    d = x - kx[j0]
    out = slope * d
    out = out + ky[j0]
    return np.where(last, ky[-1], np.where(kx[j0] == x, ky[j0], out))


def leaves_host(tables: dict, x32: np.ndarray) -> np.ndarray:
    """[n][n_trees]: the class-1 fraction of the leaf every row reaches in every tree (``x <= threshold`` goes left, the float32
    feature compared as a double)."""
    feat, right, value = tables["node_feature"], tables["node_right"].astype(np.int64), tables["node_value"]
    n = x32.shape[0]
    rows = np.arange(n)[:, None]
    k = np.broadcast_to(tables["tree_first"][:-1].astype(np.int64)[None, :], (n, tables["tree_first"].shape[0] - 1)).copy()
    for _ in range(tree_depth(tables)):
        f = feat[k]
        xv = x32[rows, np.maximum(f, 0)].astype(np.float64)
        k = np.where(f < 0, k, np.where(xv <= value[k], k + 1, right[k]))
    return value[k]


def predict_host(tables: dict, X) -> np.ndarray:
    """float64 [n]: the probability of class 1 of every row.  The same steps in the same order for every row: the leaf fractions
    of a forest's trees summed one after the other in tree order, divided by the tree count; that mean through the forest's
    calibrator; the calibrated values summed in order and divided by their count.  Without calibrators: the forest mean."""
    X = _as_rows(tables, X)
    leaves = leaves_host(tables, _to_float32(X))
    ff, cf = tables["forest_first"], tables["iso_first"]
    n_cal = cf.shape[0] - 1
    total = np.zeros(X.shape[0], dtype=np.float64)
    for c in range(ff.shape[0] - 1):
        s = np.zeros(X.shape[0], dtype=np.float64)
        for t in range(int(ff[c]), int(ff[c + 1])):
            s = s + leaves[:, t]
        mean = s / float(int(ff[c + 1]) - int(ff[c]))
        if n_cal == 0:
            return mean
        total = total + calibrate_host(mean, tables["iso_x"][cf[c]: cf[c + 1]], tables["iso_y"][cf[c]: cf[c + 1]])
    return total / float(n_cal)


# ------------------------------------------------------------------------------------------------ the device
_DECLARED = False


def _declare(lib: C.CDLL) -> None:
    global _DECLARED
    if _DECLARED:
        return
    vp, i32, pd, pi = C.c_void_p, C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_int32)
    lib.rt_forest_create.argtypes = [vp, C.POINTER(vp)]
    lib.rt_forest_destroy.argtypes = [vp]
    lib.rt_forest_set_model.argtypes = [vp, i32, i32, pi, i32, pi, i32, pi, pi, pd, i32, pi, pd, pd]
    lib.rt_forest_predict.argtypes = [vp, pd, i32, pd]
    _DECLARED = True


def set_model_raw(lib: C.CDLL, handle, t: dict) -> int:
    """``rt_forest_set_model`` on tables as they are (no Python-side validation): the status code.  ``DriftForest.set_model`` is
    the checked way in; this is for the tests of the native check."""
    _declare(lib)
    pd, pi = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    a = {k: np.ascontiguousarray(t[k], dtype=np.int32) for k in _INT_KEYS}
    a.update({k: np.ascontiguousarray(t[k], dtype=np.float64) for k in _F64_KEYS})
    return int(lib.rt_forest_set_model(
        handle, int(t["n_features"]), a["forest_first"].shape[0] - 1, a["forest_first"].ctypes.data_as(pi), a["tree_first"].shape[0] - 1,
        a["tree_first"].ctypes.data_as(pi), a["node_feature"].shape[0], a["node_feature"].ctypes.data_as(pi), a["node_right"].ctypes.data_as(pi),
        a["node_value"].ctypes.data_as(pd), a["iso_first"].shape[0] - 1, a["iso_first"].ctypes.data_as(pi), a["iso_x"].ctypes.data_as(pd),
        a["iso_y"].ctypes.data_as(pd)))


class DriftForest:
    """One ``rt_forest`` on a context: the classifier's tables in HBM, ``predict`` as one native call."""

    def __init__(self, ctx: "_native.Context", tables_or_path: Union[dict, str, None] = None):
        self.ctx, self.lib = ctx, ctx.lib
        _declare(self.lib)
        self.n_features: Optional[int] = None
        self.optimal_threshold: Optional[float] = None
        h = C.c_void_p()
        ctx.check(self.lib.rt_forest_create(ctx.handle, C.byref(h)), "rt_forest_create")
        self.handle = h
        if tables_or_path is not None:
            try:
                self.set_model(tables_or_path)
            except Exception:
                self.close()
                raise

    def close(self) -> None:
        if getattr(self, "handle", None):
            self.lib.rt_forest_destroy(self.handle)
            self.handle = None

    def set_model(self, tables_or_path: Union[dict, str]) -> None:
        """Validate and upload a model; replaces the one before it."""
        t = load(tables_or_path) if isinstance(tables_or_path, (str, bytes)) or hasattr(tables_or_path, "__fspath__") else validate(tables_or_path)
        self.ctx.check(set_model_raw(self.lib, self.handle, t), "rt_forest_set_model")
        self.n_features, self.optimal_threshold = int(t["n_features"]), float(t["optimal_threshold"])

    def predict(self, X) -> np.ndarray:
        """float64 [n]: class-1 probability of every row of ``X`` [n][n_features], bit-equal to ``predict_host``."""
        X = np.asarray(X, dtype=np.float64)
        if self.n_features is None:                                               # (the native call says so: RT_ERR_INVALID, no launch)
            self.ctx.check(self.lib.rt_forest_predict(self.handle, None, 0, None), "rt_forest_predict")
            raise ValueError("DriftForest.predict: no model set")
        if X.ndim == 1 and X.shape[0] == self.n_features:
            X = X[None, :]
        if X.ndim != 2 or X.shape[1] != self.n_features:
            raise ValueError(f"the classifier takes [n][{self.n_features}] features, got an array of shape {X.shape}")
        X = np.ascontiguousarray(X)
        out = np.zeros(X.shape[0], dtype=np.float64)
        pd = C.POINTER(C.c_double)
        self.ctx.check(self.lib.rt_forest_predict(self.handle, X.ctypes.data_as(pd), X.shape[0], out.ctypes.data_as(pd)), "rt_forest_predict")
        return out
