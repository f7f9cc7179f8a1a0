"""Writes tests/golden/forest_golden.npz: three drift classifiers fitted by scikit-learn on seeded random data, stored as exported
tables (rho_tts_amd.forest.export_sklearn) with 64 input rows each and scikit-learn's own ``predict_proba[:, 1]`` for them.

    python tests/golden/make_forest_golden.py          (CPU, needs scikit-learn; the tests that read the file need neither)

Keys, per model ``small`` / ``hand30`` / ``full``: ``<model>__<table key>`` (the format of rho_tts_amd/forest.py), ``<model>__X``
[64][n_features] float64, ``<model>__proba`` [64] float64, ``<model>__max_slope`` = the largest isotonic slope
max(diff(iso_y) / diff(iso_x)) over the calibrators, which the agreement bound needs:

    bound = 4 (n_trees + 4) 2^-53 max(1, max_slope)

(a sequential float64 sum of n_trees values in [0, 1] is off by at most (n_trees + 2) 2^-53 whatever the order; a calibrator multiplies
that by at most its largest slope).  The bound comes from what scikit-learn produced, never from the code under test, and this script
asserts that ``predict_host`` meets it before it writes the file.
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from rho_tts_amd import forest as F  # noqa: E402

OUT = os.path.join(HERE, "forest_golden.npz")
N_ROWS = 64
# name: (features, trees per forest, training rows, forest keywords)
MODELS = {
    "small": (6, 7, 400, dict(max_depth=6, min_samples_leaf=4)),
    "hand30": (30, 20, 500, dict(max_depth=8, min_samples_leaf=5)),
    "full": (286, 200, 500, dict(max_depth=10, min_samples_leaf=10, min_samples_split=20)),
}


def bound(n_trees: int, max_slope: float) -> float:
    return 4.0 * (n_trees + 4) * 2.0 ** -53 * max(1.0, float(max_slope))


def max_slope(tables: dict) -> float:
    best, first = 0.0, tables["iso_first"]
    for c in range(first.shape[0] - 1):
        x, y = tables["iso_x"][first[c]: first[c + 1]], tables["iso_y"][first[c]: first[c + 1]]
        if x.shape[0] > 1:
            best = max(best, float(np.max(np.diff(y) / np.diff(x))))
    return best


def training_data(rng: np.random.Generator, n: int, n_features: int):
    X = rng.standard_normal((n, n_features)).astype(np.float32)
    score = X[:, 0] + 0.7 * X[:, 1] - 0.5 * X[:, min(2, n_features - 1)] * X[:, min(3, n_features - 1)] + 0.8 * rng.standard_normal(n)
    return X, (score > 0.3).astype(np.int64)


def input_rows(rng: np.random.Generator, tables: dict, n_features: int) -> np.ndarray:
    X = rng.standard_normal((N_ROWS, n_features))
    # rows 40..51 sit ON a split: one feature is a stored threshold - as the float64 itself (its float32 rounding falls on either
    # side of it) and as that float32 rounding
    split = np.flatnonzero(tables["node_feature"] >= 0)
    for r, k in zip(range(40, 52), rng.choice(split, 12, replace=False)):
        thr = float(tables["node_value"][k])
        X[r, tables["node_feature"][k]] = thr if r % 2 == 0 else float(np.float32(thr))
    roots = tables["tree_first"][:-1]
    for r, k in zip(range(52, 56), roots[rng.choice(roots.shape[0], 4, replace=False)]):
        if tables["node_feature"][k] >= 0:
            X[r, tables["node_feature"][k]] = float(tables["node_value"][k])
    # rows 56..63 lie far outside the training range, to reach the calibrators' clip on both sides
    X[56], X[57], X[58], X[59] = 1.0e6, -1.0e6, 1.0e30, -1.0e30
    X[60, :2], X[61, :2], X[62, :2], X[63, :2] = 50.0, -50.0, (1.0e4, 1.0e4), (-1.0e4, -1.0e4)
    return X


def main() -> None:
    from sklearn.calibration import CalibratedClassifierCV
    from sklearn.ensemble import RandomForestClassifier
    out = {}
    for i, (name, (n_features, n_est, n_train, kw)) in enumerate(MODELS.items()):
        rng = np.random.default_rng(1000 + i)
        Xt, yt = training_data(rng, n_train, n_features)
        model = CalibratedClassifierCV(RandomForestClassifier(n_estimators=n_est, random_state=42, n_jobs=1, **kw), method="isotonic", cv=5)
        model.fit(Xt, yt)
        tables = F.export_sklearn({"model": model, "optimal_threshold": 0.2 + 0.01 * i})
        X = input_rows(rng, tables, n_features)
        proba = model.predict_proba(X)[:, 1].astype(np.float64)
        slope = max_slope(tables)
        n_trees = int(tables["forest_first"][1] - tables["forest_first"][0])
        err = float(np.max(np.abs(F.predict_host(tables, X) - proba)))
        means = F.leaves_host(tables, X.astype(np.float32)).reshape(N_ROWS, -1, n_trees).mean(axis=2)          # [rows][forests]
        lo = np.array([tables["iso_x"][a] for a in tables["iso_first"][:-1]])
        hi = np.array([tables["iso_x"][b - 1] for b in tables["iso_first"][1:]])
        below, above = int(np.count_nonzero(means < lo[None, :])), int(np.count_nonzero(means > hi[None, :]))
        assert below > 0 and above > 0, (name, "no row reaches the clip", below, above)
        print(f"{name}: {tables['node_feature'].shape[0]} nodes, depth {F.tree_depth(tables)}, {tables['iso_x'].shape[0]} knots, max slope {slope:.1f}, "
              f"|host - sklearn| {err:.2e} (bound {bound(n_trees, slope):.2e}), {below} / {above} forest means clipped below / above")
        assert err <= bound(n_trees, slope), (name, err, bound(n_trees, slope))
        for k in F.KEYS:
            out[f"{name}__{k}"] = tables[k]
        out[f"{name}__X"], out[f"{name}__proba"], out[f"{name}__max_slope"] = X, proba, np.float64(slope)
    np.savez_compressed(OUT, **out)
    print(f"{OUT}: {os.path.getsize(OUT)} bytes")
    assert os.path.getsize(OUT) < 1 << 20


if __name__ == "__main__":
    main()
