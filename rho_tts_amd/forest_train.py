"""Training the accent-drift classifier on this build's own feature vectors (the trainer half).

The reference fits ``CalibratedClassifierCV(RandomForestClassifier(200, max_depth=10, min_samples_leaf=10, min_samples_split=20,
max_features='sqrt', class_weight=...), isotonic, cv=5)`` on librosa / resemblyzer vectors and sweeps a cost-sensitive threshold
(validation/classifier/trainer.py:201-251).  This module fits the same model family on the rows inference will see
(``features.forest_rows``), writes the version-1 tables of ``forest.py`` directly, and imports neither scikit-learn nor pickle.

``fit_host`` is the definition of the kernels of csrc/forest_fit.hip (``rt_forest_fit``, ``fit_device``): the device tables equal
its tables bit for bit, as ``forest.predict_host`` is the definition of csrc/forest.hip.  The rules, which are the contract:

Inputs.  ``X`` [n][F] float64 is rounded to float32 and refused when that is not finite (``forest._to_float32``); every comparison
  is on ``(double)float32``, which is what inference compares.  ``y`` [n] holds 0 / 1.  ``member`` [n_forests][n] uint8: row i takes
  part in forest c.  ``FitParams``: n_trees (per forest), max_depth, min_samples_leaf, min_samples_split, max_features (None:
  floor(sqrt(F)), at least 1), w0 / w1 (class weights, float64, positive), seed (u64), bootstrap (default on).

Random numbers.  Every random number is a murmur3 fmix32 counter hash (``mix32``), the family of rt_uniform and weights._mix32; all
  sums are modulo 2^32.  A draw in [0, m) is ``(hash * m) >> 32`` in 64-bit integers.
    tree key   T = mix32(mix32(mix32(mix32(seed_lo ^ 0x85EBCA6B) + seed_hi * 0x9E3779B1) + c * 0x85EBCA77) + t * 0xC2B2AE3D)
    bootstrap  draw j of (forest c, tree t) = mix32(mix32(T + 0x9E3779B1) + j * 0x85EBCA77)
    node key   root = mix32(T + 0x3C6EF362); child = mix32(parent + (1 left | 2 right) * 0xC2B2AE3D)
    features   draw j of a node = mix32((node key ^ 0x68E31DA4) + j * 0x85EBCA77)
  Nothing depends on the launch shape, on the other trees of the call or on the order in which nodes are visited.

Bootstrap.  With m = the forest's member count, m draws over the member rows (in ascending row order) give a multiplicity c[i]; rows
  with c[i] == 0 are out of the tree.  ``bootstrap=False``: every member row has multiplicity 1.

A node is a set of distinct rows: m = their number, M0 / M1 = the integer multiplicity sums per class, W0 = w0 * M0 and W1 = w1 * M1
  (ONE multiplication from an exact integer each, so the result is reproducible whatever the weights are).  It is a leaf when
  depth == max_depth, or m < min_samples_split, or m < 2 * min_samples_leaf, or M0 == 0, or M1 == 0, or no valid candidate exists.
  Leaf value = W1 / (W0 + W1).  min_samples_* count distinct rows, as scikit-learn does with bootstrap weights.

Candidate features.  max_features distinct features by a partial Fisher-Yates over 0 .. F-1 (step j swaps entry j with entry
  j + draw_j(F - j)), examined in draw order.  DEVIATION: exactly max_features features are examined; scikit-learn goes on drawing
  while none of them yields a split.

Split search for feature f.  The node's rows ordered by (float32 value, row index).  The boundary after sorted position p is valid
  when v[p] != v[p + 1] and both sides hold at least min_samples_leaf distinct rows.  With L0 = w0 * ML0, L1 = w1 * ML1,
  R0 = w0 * MR0, R1 = w1 * MR1 the score is (L0*L0 + L1*L1) / (L0 + L1) + (R0*R0 + R1*R1) / (R0 + R1) in exactly that operation
  order, float64, unfused.  The best split has the largest score; ties go to the earlier feature in draw order, then to the lower
  position.  Threshold = (double)v[p] / 2 + (double)v[p + 1] / 2 (exact, strictly between the two); ``x <= threshold`` goes left.

Output.  Format version 1 tables of forest.py: pre-order nodes with left child = k + 1, n_forests forests, no calibrators.

The rest - ``split_train_test``, ``folds``, ``isotonic_fit``, the class weights, the threshold sweep, the Brier score, ``train`` - is
host code, deterministic, and free of random numbers except the split's hash.
"""
from __future__ import annotations

import ctypes as C
import json
import logging
import math
import os
import wave
from dataclasses import dataclass
from datetime import datetime
from typing import Callable, List, Optional, Sequence, Tuple

import numpy as np

from . import forest as F

logger = logging.getLogger(__name__)

MAX_ROWS = 16384                                   # rank tables hold 16-bit positions; one LDS slot per row
MAX_FEATURES = 1024
CV = 5
FN_COST, FP_COST = 5.0, 1.0                        # trainer.py:210-211
CHUNK = 32                                         # clips per feature call
_M = 0xFFFFFFFF


# ------------------------------------------------------------------------------------------------ the generator
def mix32(h):
    """murmur3's fmix32 on a Python int or a uint64 array (values below 2^32 on return)."""
    h = h & _M
    h = h ^ (h >> 16)
    h = (h * 0x85EBCA6B) & _M
    h = h ^ (h >> 13)
    h = (h * 0xC2B2AE35) & _M
    return h ^ (h >> 16)


def tree_key(seed: int, c: int, t: int) -> int:
    h = mix32((seed & _M) ^ 0x85EBCA6B)
    h = mix32(h + ((seed >> 32) & _M) * 0x9E3779B1)
    h = mix32(h + c * 0x85EBCA77)
    return mix32(h + t * 0xC2B2AE3D)


def bootstrap_draws(tkey: int, m: int) -> np.ndarray:
    """The m draws in [0, m) of a tree's bootstrap, int64."""
    bk = mix32(tkey + 0x9E3779B1)
    j = np.arange(m, dtype=np.uint64)
    h = mix32(np.uint64(bk) + j * np.uint64(0x85EBCA77))
    return ((h * np.uint64(m)) >> np.uint64(32)).astype(np.int64)


def root_key(tkey: int) -> int:
    return mix32(tkey + 0x3C6EF362)


def child_key(key: int, right: int) -> int:
    return mix32(key + (2 if right else 1) * 0xC2B2AE3D)


def feature_draws(key: int, n_features: int, k: int) -> List[int]:
    """k distinct features of a node in draw order: a partial Fisher-Yates over 0 .. n_features - 1."""
    perm = list(range(n_features))
    base = key ^ 0x68E31DA4
    for j in range(k):
        r = j + ((mix32(base + j * 0x85EBCA77) * (n_features - j)) >> 32)
        perm[j], perm[r] = perm[r], perm[j]
    return perm[:k]


# ------------------------------------------------------------------------------------------------ the definition of the fit
@dataclass
class FitParams:
    n_trees: int = 200
    max_depth: int = 10
    min_samples_leaf: int = 10
    min_samples_split: int = 20
    max_features: Optional[int] = None             # None: floor(sqrt(F)), at least 1
    w0: float = 1.0
    w1: float = 1.0
    seed: int = 42
    bootstrap: bool = True

    def features_per_node(self, n_features: int) -> int:
        return max(1, math.isqrt(n_features)) if self.max_features is None else int(self.max_features)


def tree_capacity(params: FitParams, n_members: int) -> int:
    """The node bound of one tree over n_members rows (the capacity rule of include/rho_tts_amd.h): every leaf of a tree with more
    than one node holds at least min_samples_leaf distinct rows, and a tree of depth d has at most 2^(d + 1) - 1 nodes."""
    by_rows = max(1, 2 * (n_members // max(1, int(params.min_samples_leaf))) - 1)
    return int(min(by_rows, 2 ** (min(int(params.max_depth), 30) + 1) - 1))


def _check_inputs(X, y, member, params: FitParams):
    X = np.asarray(X, dtype=np.float64)
    if X.ndim != 2 or X.shape[0] < 1 or X.shape[1] < 1:
        raise ValueError(f"fit: X must be [n][F], got an array of shape {X.shape}")
    n, nf = X.shape
    if n > MAX_ROWS or nf > MAX_FEATURES:
        raise ValueError(f"fit: {n} rows of {nf} features (at most {MAX_ROWS} rows, {MAX_FEATURES} features)")
    x32 = F._to_float32(np.ascontiguousarray(X))
    y = np.asarray(y)
    if y.shape != (n,) or not np.all((y == 0) | (y == 1)):
        raise ValueError("fit: y must be [n] with values 0 and 1")
    y = y.astype(np.uint8)
    member = np.asarray(member)
    if member.ndim != 2 or member.shape[1] != n or not 1 <= member.shape[0] <= F.MAX_FORESTS:
        raise ValueError(f"fit: member must be [n_forests][{n}] with 1 .. {F.MAX_FORESTS} forests, got shape {member.shape}")
    member = np.ascontiguousarray(member != 0, dtype=np.uint8)
    if np.any(member.sum(axis=1) == 0):
        raise ValueError("fit: a forest without member rows")
    mf = params.features_per_node(nf)
    if not (1 <= int(params.n_trees) and 0 <= int(params.max_depth) <= F.MAX_DEPTH and int(params.min_samples_leaf) >= 1
            and int(params.min_samples_split) >= 2 and 1 <= mf <= nf):
        raise ValueError(f"fit: parameters out of range ({params}, {nf} features)")
    if not (np.isfinite(params.w0) and np.isfinite(params.w1) and params.w0 > 0 and params.w1 > 0):
        raise ValueError("fit: class weights must be positive and finite")
    if not 0 <= int(params.seed) < 2 ** 64:
        raise ValueError("fit: the seed is a 64-bit unsigned integer")
    return x32, y, member, mf


def column_ranks(x32: np.ndarray) -> np.ndarray:
    """[F][n]: the position of every row in the order of its column by (float32 value, row index)."""
    n, nf = x32.shape
    rank = np.empty((nf, n), dtype=np.int64)
    ar = np.arange(n)
    for f in range(nf):
        rank[f, np.argsort(x32[:, f], kind="stable")] = ar
    return rank


def _best_split(v: np.ndarray, c0: np.ndarray, c1: np.ndarray, m: int, msl: int, w0: float, w1: float):
    """(score, position) of the best boundary of one feature, or None.  v: the values in order; c0 / c1: inclusive prefix
    multiplicities per class."""
    p = np.arange(m - 1)
    ok = (v[:-1] != v[1:]) & (p + 1 >= msl) & (m - (p + 1) >= msl)
    if not ok.any():
        return None
    p = p[ok]
    l0, l1 = w0 * c0[p].astype(np.float64), w1 * c1[p].astype(np.float64)
    r0, r1 = w0 * (c0[-1] - c0[p]).astype(np.float64), w1 * (c1[-1] - c1[p]).astype(np.float64)
    score = (l0 * l0 + l1 * l1) / (l0 + l1) + (r0 * r0 + r1 * r1) / (r0 + r1)
    k = int(np.argmax(score))                                                      # the first of equal scores: the lower position
    return float(score[k]), int(p[k])


def _fit_tree(x32: np.ndarray, rank: np.ndarray, y: np.ndarray, rows: np.ndarray, mult: np.ndarray, params: FitParams, mf: int, tkey: int):
    """One tree in pre-order: (feature, right child (tree-local), value) lists."""
    nf = x32.shape[1]
    w0, w1, msl = float(params.w0), float(params.w1), int(params.min_samples_leaf)
    feat, right, value = [], [], []
    stack = [(rows, 0, root_key(tkey), -1)]                                        # rows, depth, key, the parent this is the right child of
    while stack:
        rows, depth, key, parent = stack.pop()
        k = len(feat)
        if parent >= 0:
            right[parent] = k
        m = rows.shape[0]
        mu, cls = mult[rows], y[rows]
        m1 = int(mu[cls == 1].sum())
        m0 = int(mu.sum()) - m1
        best = None
        if not (depth == params.max_depth or m < params.min_samples_split or m < 2 * msl or m0 == 0 or m1 == 0):
            for f in feature_draws(key, nf, mf):
                o = np.argsort(rank[f, rows])
                rs = rows[o]
                mo, co = mult[rs], y[rs]
                c1 = np.cumsum(np.where(co == 1, mo, 0))
                c0 = np.cumsum(mo) - c1
                v = x32[rs, f]
                got = _best_split(v, c0, c1, m, msl, w0, w1)
                if got is not None and (best is None or got[0] > best[0]):
                    best = (got[0], f, rs, got[1], v)
        if best is None:
            feat.append(-1)
            right.append(-1)
            value.append((w1 * float(m1)) / (w0 * float(m0) + w1 * float(m1)))
            continue
        _, f, rs, p, v = best
        feat.append(f)
        right.append(-1)
        value.append(float(np.float64(v[p]) / 2.0 + np.float64(v[p + 1]) / 2.0))
        stack.append((rs[p + 1:], depth + 1, child_key(key, 1), k))
        stack.append((rs[: p + 1], depth + 1, child_key(key, 0), -1))
    return feat, right, value


def tree_rows(member_rows: np.ndarray, n: int, params: FitParams, tkey: int) -> Tuple[np.ndarray, np.ndarray]:
    """(the distinct rows of a tree, ascending; the multiplicity of every row of the data set)."""
    mult = np.zeros(n, dtype=np.int64)
    if params.bootstrap:
        np.add.at(mult, member_rows[bootstrap_draws(tkey, member_rows.shape[0])], 1)
    else:
        mult[member_rows] = 1
    return np.flatnonzero(mult), mult


def assemble(n_features: int, n_forests: int, n_trees: int, trees) -> dict:
    """Version-1 tables without calibrators from per-tree (feature, tree-local right child, value) triples, forest by forest.  One
    forest: validated as it is.  Several forests without calibrators are not a servable model (``forest.validate`` refuses them), so
    each is validated on its own as bare tables; ``with_calibrators`` makes the servable whole."""
    tree_first, feat, right, value = [0], [], [], []
    for f, r, v in trees:
        base = tree_first[-1]
        r = np.asarray(r, dtype=np.int64)
        feat.append(np.asarray(f, dtype=np.int32))
        right.append(np.where(r >= 0, r + base, -1).astype(np.int32))
        value.append(np.asarray(v, dtype=np.float64))
        tree_first.append(base + len(f))
    t = {"version": np.int32(F.FORMAT_VERSION), "n_features": np.int32(n_features), "optimal_threshold": np.float64(F.DEFAULT_OPTIMAL_THRESHOLD),
         "forest_first": np.arange(n_forests + 1, dtype=np.int32) * np.int32(n_trees), "tree_first": np.asarray(tree_first, dtype=np.int32),
         "node_feature": np.concatenate(feat), "node_right": np.concatenate(right), "node_value": np.concatenate(value),
         "iso_first": np.zeros(1, dtype=np.int32), "iso_x": np.zeros(0), "iso_y": np.zeros(0)}
    if n_forests == 1:
        return F.validate(t)
    for c in range(n_forests):
        single_forest(t, c)
    return t


def single_forest(tables: dict, c: int) -> dict:
    """Forest c of a fit as bare single-forest tables (validated): what ``DriftForest.predict`` / ``predict_host`` take to give the
    forest's mean."""
    ff, tf = tables["forest_first"], tables["tree_first"]
    t0, t1 = int(ff[c]), int(ff[c + 1])
    k0, k1 = int(tf[t0]), int(tf[t1])
    right = tables["node_right"][k0:k1].astype(np.int64)
    return F.validate({
        "version": np.int32(F.FORMAT_VERSION), "n_features": tables["n_features"], "optimal_threshold": tables["optimal_threshold"],
        "forest_first": np.asarray([0, t1 - t0], dtype=np.int32), "tree_first": (tf[t0: t1 + 1].astype(np.int64) - k0).astype(np.int32),
        "node_feature": tables["node_feature"][k0:k1], "node_right": np.where(right >= 0, right - k0, -1).astype(np.int32),
        "node_value": tables["node_value"][k0:k1], "iso_first": np.zeros(1, dtype=np.int32), "iso_x": np.zeros(0), "iso_y": np.zeros(0)})


def with_calibrators(tables: dict, knots: Sequence[Tuple[np.ndarray, np.ndarray]], optimal_threshold: float) -> dict:
    """The fitted forests with one isotonic calibrator each and the threshold: a servable model (validated)."""
    t = dict(tables)
    first = [0]
    for kx, _ in knots:
        first.append(first[-1] + int(kx.shape[0]))
    t["iso_first"] = np.asarray(first, dtype=np.int32)
    t["iso_x"] = np.concatenate([np.asarray(kx, dtype=np.float64) for kx, _ in knots])
    t["iso_y"] = np.concatenate([np.asarray(ky, dtype=np.float64) for _, ky in knots])
    t["optimal_threshold"] = np.float64(optimal_threshold)
    return F.validate(t)


def fit_host(X, y, member, params: FitParams) -> dict:
    """The forests of ``member``'s rows as version-1 tables without calibrators: the definition ``rt_forest_fit`` equals bit for bit.
    One forest: validated bare tables.  Several: every forest is validated on its own (``single_forest``); ``with_calibrators``
    makes the servable model."""
    x32, y, member, mf = _check_inputs(X, y, member, params)
    n, nf = x32.shape
    rank = column_ranks(x32)
    trees = []
    for c in range(member.shape[0]):
        member_rows = np.flatnonzero(member[c])
        for t in range(int(params.n_trees)):
            tkey = tree_key(int(params.seed), c, t)
            rows, mult = tree_rows(member_rows, n, params, tkey)
            trees.append(_fit_tree(x32, rank, y, rows, mult, params, mf, tkey))
    return assemble(nf, member.shape[0], int(params.n_trees), trees)


# ------------------------------------------------------------------------------------------------ the device
class _RtFitParams(C.Structure):
    _fields_ = [("n_trees", C.c_int32), ("max_depth", C.c_int32), ("min_samples_leaf", C.c_int32), ("min_samples_split", C.c_int32),
                ("max_features", C.c_int32), ("bootstrap", C.c_int32), ("w0", C.c_double), ("w1", C.c_double), ("seed", C.c_uint64)]


def fit_raw(ctx, X: np.ndarray, y: np.ndarray, member: np.ndarray, params: FitParams, node_cap: Optional[int] = None):
    """``rt_forest_fit`` on arrays as they are (no Python-side checks): (status, tree_first, node_feature, node_right, node_value),
    the node arrays cut to the returned count.  ``fit_device`` is the checked way in; this is for the tests of the refusals."""
    lib = ctx.lib
    pd, pi, pb = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
    lib.rt_forest_fit.argtypes = [C.c_void_p, pd, C.c_int32, C.c_int32, pb, pb, C.c_int32, C.POINTER(_RtFitParams), C.c_int32, pi, pi, pi, pd, pi]
    lib.rt_forest_fit.restype = C.c_int
    X = np.ascontiguousarray(X, dtype=np.float64)
    y = np.ascontiguousarray(y, dtype=np.uint8)
    member = np.ascontiguousarray(member, dtype=np.uint8)
    n, nf = X.shape
    n_forests = member.shape[0]
    n_trees = n_forests * int(params.n_trees)
    if node_cap is None:
        node_cap = int(sum(tree_capacity(params, int(np.count_nonzero(member[c]))) for c in range(n_forests)) * int(params.n_trees))
    p = _RtFitParams(int(params.n_trees), int(params.max_depth), int(params.min_samples_leaf), int(params.min_samples_split),
                     0 if params.max_features is None else int(params.max_features), 1 if params.bootstrap else 0,
                     float(params.w0), float(params.w1), int(params.seed))
    tree_first = np.zeros(max(n_trees, 0) + 1, dtype=np.int32)
    feat = np.zeros(max(node_cap, 1), dtype=np.int32)
    right = np.zeros(max(node_cap, 1), dtype=np.int32)
    value = np.zeros(max(node_cap, 1), dtype=np.float64)
    n_nodes = C.c_int32(0)
    rc = int(lib.rt_forest_fit(ctx.handle, X.ctypes.data_as(pd), n, nf, y.ctypes.data_as(pb), member.ctypes.data_as(pb), n_forests, C.byref(p),
                               int(node_cap), tree_first.ctypes.data_as(pi), feat.ctypes.data_as(pi), right.ctypes.data_as(pi),
                               value.ctypes.data_as(pd), C.byref(n_nodes)))
    k = int(n_nodes.value)
    return rc, tree_first, feat[:k], right[:k], value[:k]


def fit_device(ctx, X, y, member, params: FitParams) -> dict:
    """``fit_host`` on the GPU: one ``rt_forest_fit`` call, the same tables bit for bit."""
    _check_inputs(X, y, member, params)
    X = np.asarray(X, dtype=np.float64)
    member = np.asarray(member) != 0
    rc, tree_first, feat, right, value = fit_raw(ctx, X, np.asarray(y), member, params)
    ctx.check(rc, "rt_forest_fit")
    n_forests = member.shape[0]
    trees = []
    for t in range(tree_first.shape[0] - 1):
        k0, k1 = int(tree_first[t]), int(tree_first[t + 1])
        r = right[k0:k1].astype(np.int64)
        trees.append((feat[k0:k1], np.where(r >= 0, r - k0, -1), value[k0:k1]))
    return assemble(X.shape[1], n_forests, int(params.n_trees), trees)


# ------------------------------------------------------------------------------------------------ the trainer's host steps
def split_train_test(y, seed: int) -> Tuple[np.ndarray, np.ndarray]:
    """Stratified 80 / 20: (train rows, test rows), each ascending.  Per class the rows are ranked by hash(seed, row) (ties by row);
    the first round(0.2 * n_class) go to the test set."""
    y = np.asarray(y)
    s = mix32(mix32((seed & _M) ^ 0x85EBCA6B) + ((seed >> 32) & _M) * 0x9E3779B1)
    test = []
    for cls in (0, 1):
        rows = np.flatnonzero(y == cls)
        h = mix32(np.uint64(s) + rows.astype(np.uint64) * np.uint64(0x85EBCA77))
        order = rows[np.lexsort((rows, h))]
        test.append(order[: int(math.floor(0.2 * rows.shape[0] + 0.5))])
    test = np.sort(np.concatenate(test))
    return np.setdiff1d(np.arange(y.shape[0]), test), test


def folds(y_train, cv: int = CV) -> np.ndarray:
    """[n]: the fold of every training row - the j-th row of its class, in data-set order, goes to fold j % cv.  Forest c is fitted
    on the rows outside fold c.  A class with fewer than cv rows is a ``ValueError``."""
    y_train = np.asarray(y_train)
    fold = np.zeros(y_train.shape[0], dtype=np.int64)
    for cls in (0, 1):
        rows = np.flatnonzero(y_train == cls)
        if rows.shape[0] < cv:
            raise ValueError(f"class {cls} ({'good' if cls == 0 else 'bad'}) has {rows.shape[0]} rows in the training split, fewer than the "
                             f"{cv} folds of the calibration (the split holds {int(np.sum(y_train == 0))} good and {int(np.sum(y_train == 1))} bad)")
        fold[rows] = np.arange(rows.shape[0]) % cv
    return fold


def isotonic_fit(x, y) -> Tuple[np.ndarray, np.ndarray]:
    """The knots (kx, ky) of scikit-learn's ``IsotonicRegression(out_of_bounds='clip')`` as ``_CalibratedClassifier`` fits it: sort by
    (x, y); pool equal x by their mean (x closer than 1e-15 to the first of a run count as equal, scikit-learn's rule); pool
    adjacent violators; keep only the knots at the ends of constant runs; y clipped to [0, 1]."""
    x, y = np.asarray(x, dtype=np.float64).reshape(-1), np.asarray(y, dtype=np.float64).reshape(-1)
    if x.shape[0] < 1 or x.shape != y.shape or not (np.all(np.isfinite(x)) and np.all(np.isfinite(y))):
        raise ValueError("isotonic_fit: x and y must be finite, of one length, and not empty")
    order = np.lexsort((y, x))
    x, y = x[order], y[order]
    ux, sy, sw = [], [], []                                                        # unique x, sum of y, count
    for xv, yv in zip(x.tolist(), y.tolist()):
        if ux and xv - ux[-1] < 1e-15:
            sy[-1] += yv
            sw[-1] += 1.0
        else:
            ux.append(xv)
            sy.append(yv)
            sw.append(1.0)
    blocks: list = []                                                              # [sum of weight * y, weight, points]
    for s, w in zip(sy, sw):
        blocks.append([(s / w) * w, w, 1])
        while len(blocks) > 1 and blocks[-2][0] / blocks[-2][1] >= blocks[-1][0] / blocks[-1][1]:
            b = blocks.pop()
            blocks[-1][0] += b[0]
            blocks[-1][1] += b[1]
            blocks[-1][2] += b[2]
    fy = np.concatenate([np.full(b[2], b[0] / b[1]) for b in blocks])
    fy = np.clip(fy, 0.0, 1.0)
    kx = np.asarray(ux, dtype=np.float64)
    keep = np.ones(fy.shape[0], dtype=bool)
    keep[1:-1] = (fy[1:-1] != fy[:-2]) | (fy[1:-1] != fy[2:])
    return kx[keep], fy[keep]


def class_weights(y_train) -> Tuple[float, float]:
    """(w0, w1) as trainer.py:208-215: balanced weights times the cost of missing that class."""
    y_train = np.asarray(y_train)
    n_good, n_bad, total = int(np.sum(y_train == 0)), int(np.sum(y_train == 1)), int(y_train.shape[0])
    return (total / (2 * n_good)) * FN_COST, (total / (2 * n_bad)) * FP_COST


def threshold_sweep(probs, y_test) -> Tuple[float, float]:
    """(optimal threshold, expected cost): 0.01 .. 0.99 with the reference's strict ``<`` update (trainer.py:236-249)."""
    probs, y_test = np.asarray(probs, dtype=np.float64), np.asarray(y_test)
    best_cost, best = float("inf"), F.DEFAULT_OPTIMAL_THRESHOLD
    for thresh in np.arange(0.01, 1.0, 0.01):
        pred = probs >= thresh
        fp = int(np.sum((y_test == 0) & pred))
        fn = int(np.sum((y_test == 1) & ~pred))
        cost = (fn * FN_COST + fp * FP_COST) / y_test.shape[0]
        if cost < best_cost:
            best_cost, best = cost, float(thresh)
    return best, best_cost


def brier_score(probs, y_test) -> float:
    probs, y_test = np.asarray(probs, dtype=np.float64), np.asarray(y_test, dtype=np.float64)
    return float(np.mean((probs - y_test) ** 2))


def fit_classifier(X, y, *, seed: int = 42, fit=fit_host, predict=F.predict_host, n_trees: int = 200) -> Tuple[dict, dict]:
    """The trainer's model from rows and labels: (servable tables, metadata).  ``fit(X, y, member, params) -> tables`` and
    ``predict(tables, X) -> probabilities`` are the host definitions by default; ``train`` hands in the device calls."""
    X, y = np.asarray(X, dtype=np.float64), np.asarray(y).astype(np.int64)
    train_rows, test_rows = split_train_test(y, seed)
    Xt, yt = X[train_rows], y[train_rows]
    fold = folds(yt, CV)
    w0, w1 = class_weights(yt)
    params = FitParams(n_trees=n_trees, w0=w0, w1=w1, seed=seed)
    member = np.stack([(fold != c) for c in range(CV)]).astype(np.uint8)
    forests = fit(Xt, yt, member, params)
    knots = []
    for c in range(CV):
        held = fold == c
        knots.append(isotonic_fit(predict(single_forest(forests, c), Xt[held]), yt[held]))
    model = with_calibrators(forests, knots, F.DEFAULT_OPTIMAL_THRESHOLD)
    probs = predict(model, X[test_rows])
    threshold, cost = threshold_sweep(probs, y[test_rows])
    model = with_calibrators(forests, knots, threshold)
    meta = {"model_name": "RandomForest", "optimal_threshold": threshold, "fn_cost": FN_COST, "fp_cost": FP_COST,
            "training_date": datetime.now().isoformat(), "class_distribution": {"good": int(np.sum(y == 0)), "bad": int(np.sum(y == 1))},
            "expected_cost": cost, "brier_score": brier_score(probs, y[test_rows]), "n_features": int(X.shape[1]), "seed": int(seed)}
    return model, meta


# ------------------------------------------------------------------------------------------------ the public trainer
def read_wav(path: str) -> Tuple[np.ndarray, int]:
    """(float32 samples in [-1, 1), sample rate) of a PCM16 file at any rate; channels are averaged."""
    with wave.open(path, "rb") as w:
        if w.getsampwidth() != 2 or w.getcomptype() != "NONE":
            raise ValueError(f"{path}: not 16-bit PCM")
        ch, sr, raw = w.getnchannels(), w.getframerate(), w.readframes(w.getnframes())
    a = np.frombuffer(raw, dtype="<i2").astype(np.float32) / 32768.0
    if ch > 1:
        a = a[: a.shape[0] // ch * ch].reshape(-1, ch).mean(axis=1).astype(np.float32)
    if a.shape[0] < 2:
        raise ValueError(f"{path}: fewer than two samples")
    return a, int(sr)


def default_output_path(voice_id: Optional[str]) -> str:
    if voice_id is not None:
        models_dir = os.path.join(os.path.expanduser("~"), ".rho_tts", "models")
        os.makedirs(models_dir, exist_ok=True)
        return os.path.join(models_dir, f"{voice_id}_classifier.npz")
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "voice_quality_model.npz")


def train(dataset_dir: str, voice_id: Optional[str] = None, output_path: Optional[str] = None,
          progress_callback: Optional[Callable[[str], None]] = None, *, ctx=None, speaker_encoder_path: Optional[str] = None, seed: int = 42,
          features: Optional[Callable[[Sequence, int], np.ndarray]] = None, embed=None) -> str:
    """Train the drift classifier of ``dataset_dir`` (``good/*.wav``, ``bad/*.wav``) on this build's own feature vectors and write it
    as version-1 tables (``.npz``) with a ``.json`` of the reference's metadata beside it; returns the path.  The reference's
    signature, progress strings and errors (trainer.py:112-270).  The default output is ``~/.rho_tts/models/{voice_id}_classifier.npz``.

    ``ctx``: the native context to run on (one is made on GPU 0, and closed, when none is given).  With ``speaker_encoder_path`` the
    rows are [256 GE2E | 30 hand-crafted], without it the 30 alone.  ``embed``: a caller's own batch embedding callable in place of
    that encoder (the provider hands in its own).  ``features``: a callable
    ``(clips, sample_rate) -> [n][F]`` in place of all of that; the forests are then fitted by the host definition, and no GPU is
    touched."""
    def say(msg: str) -> None:
        logger.info(msg)
        if progress_callback:
            progress_callback(msg)

    if output_path is None:
        output_path = default_output_path(voice_id)
    logger.info("Voice Quality Classifier Training")
    listing = {}
    for folder in ("good", "bad"):
        fp = os.path.join(dataset_dir, folder)
        if os.path.exists(fp):
            listing[folder] = [f for f in sorted(os.listdir(fp)) if f.endswith(".wav")]
    total_files = sum(len(v) for v in listing.values())

    own_ctx, own = None, []
    try:
        if features is None:
            from .features import HandcraftedFeatures, forest_rows
            if ctx is None:
                import torch  # noqa: F401  (before the library: one HIP runtime per process)
                from . import _native
                ctx = own_ctx = _native.Context(0)
            extractor = HandcraftedFeatures(ctx)
            own.append(extractor)
            if embed is None and speaker_encoder_path:
                from .speaker import SpeakerEmbedder
                embed = SpeakerEmbedder(ctx, str(speaker_encoder_path))
                own.append(embed)

            def features(clips, sr):
                return forest_rows(extractor, embed, clips, sr)

        X, y, file_index = [], [], 0
        for label, folder in enumerate(("good", "bad")):
            folder_path = os.path.join(dataset_dir, folder)
            if not os.path.exists(folder_path):
                raise FileNotFoundError(f"Dataset folder not found: {folder_path}")
            logger.info(f"Loading from: {folder_path}")
            wav_files, count = listing[folder], 0
            pending: list = []                                                     # clips of one sample rate, at most CHUNK

            def flush():
                nonlocal count
                if pending:
                    try:
                        rows = np.asarray(features([a for a, _ in pending], pending[0][1]), dtype=np.float64).reshape(len(pending), -1)
                        F._to_float32(rows)
                        X.extend(rows)
                        y.extend([label] * len(pending))
                        count += len(pending)
                    except Exception as e:                                         # (one bad clip must not cost its chunk: clip by clip)
                        for a, sr in pending:
                            try:
                                row = np.asarray(features([a], sr), dtype=np.float64).reshape(-1)
                                F._to_float32(row)
                                X.append(row)
                                y.append(label)
                                count += 1
                            except Exception as e1:
                                logger.error(f"Error processing a clip of {folder}/: {e1} (chunk: {e})")
                    pending.clear()

            for i, f in enumerate(wav_files):
                file_index += 1
                try:
                    a, sr = read_wav(os.path.join(folder_path, f))
                    if pending and (pending[0][1] != sr or len(pending) == CHUNK):
                        flush()
                    pending.append((a, sr))
                except Exception as e:
                    logger.error(f"Error processing {os.path.join(folder_path, f)}: {e}")
                is_last = i == len(wav_files) - 1
                if is_last:
                    flush()
                pct = file_index * 100 // total_files if total_files else 0
                if file_index % 10 == 0 or is_last:
                    say(f"Extracting: {file_index}/{total_files} ({pct}%) — {folder}/{f}")
            say(f"Loaded {count} files from {folder}/")

        n_good, n_bad = y.count(0), y.count(1)
        say(f"Loaded {len(X)} samples ({n_good} good, {n_bad} bad)")
        if len(X) < 5:
            raise ValueError(f"Not enough samples to train a classifier (found {len(X)}, need at least 5). "
                             f"Add .wav files to {dataset_dir}/good/ and {dataset_dir}/bad/.")
        X, y = np.stack(X), np.asarray(y, dtype=np.int64)
        if progress_callback:
            progress_callback("Training model (this may take a moment)...")
        forest_handle = None
        if ctx is not None:
            forest_handle = F.DriftForest(ctx)
            own.append(forest_handle)

            def predict(tables, rows):
                forest_handle.set_model(tables)
                return forest_handle.predict(rows)
            model, meta = fit_classifier(X, y, seed=seed, fit=lambda *a: fit_device(ctx, *a), predict=predict)
        else:
            model, meta = fit_classifier(X, y, seed=seed)
        logger.info("Training completed!")
        if progress_callback:
            progress_callback("Training complete! Optimizing threshold...")
            progress_callback(f"Optimal threshold: {meta['optimal_threshold']:.3f}")
        from . import _build
        meta["native_source_hash"] = _build.source_hash()
        F.save(output_path, model)
        with open(os.path.splitext(output_path)[0] + ".json", "w") as fh:
            json.dump(meta, fh, indent=1)
        say(f"Model saved to {output_path} (threshold: {meta['optimal_threshold']:.3f}, brier: {meta['brier_score']:.4f})")
        return output_path
    finally:
        for h in reversed(own):
            h.close()
        if own_ctx is not None:
            own_ctx.close()
