"""What the drift-classifier tests share (tests/test_forest_cpu.py, tests/test_forest_gpu.py): the golden models of
tests/golden/forest_golden.npz (tests/golden/make_forest_golden.py wrote it with scikit-learn), the agreement bound, the hand-built
edge trees with the values they must give, and the malformed tables ``validate`` and the native check must refuse."""
from __future__ import annotations

import functools
import os

import numpy as np

from rho_tts_amd import forest as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "forest_golden.npz")
MODELS = ("small", "hand30", "full")


@functools.lru_cache(maxsize=None)
def golden(name: str):
    """(tables, X [64][n_features], scikit-learn's predict_proba[:, 1] [64], bound, predict_host(tables, X)) - computed once, read-only."""
    with np.load(GOLDEN, allow_pickle=False) as z:
        tables = F.validate({k: z[f"{name}__{k}"] for k in F.KEYS})
        X, proba, slope = z[f"{name}__X"], z[f"{name}__proba"], float(z[f"{name}__max_slope"])
    n_trees = int(tables["forest_first"][1] - tables["forest_first"][0])
    host = F.predict_host(tables, X)
    for a in (X, proba, host, *tables.values()):
        if isinstance(a, np.ndarray) and a.ndim:
            a.setflags(write=False)
    return tables, X, proba, bound(n_trees, slope), host


def bound(n_trees: int, max_slope: float) -> float:
    """Derived, not tuned: a sequential float64 sum of n_trees values in [0, 1] is off by at most (n_trees + 2) 2^-53 whatever the
    order; the calibrator multiplies that by at most its largest slope."""
    return 4.0 * (n_trees + 4) * 2.0 ** -53 * max(1.0, float(max_slope))


def tables_of(n_features: int, forests, calibrators=(), optimal_threshold: float = F.DEFAULT_OPTIMAL_THRESHOLD) -> dict:
    """Tables from ``forests`` = lists of trees = lists of nodes (feature or -1, threshold / leaf value, right child within the
    tree or -1) and ``calibrators`` = (knot x, knot y) per forest.  Not validated: the malformed cases are built with it too."""
    forest_first, tree_first, feat, value, right = [0], [0], [], [], []
    for trees in forests:
        for tree in trees:
            base = tree_first[-1]
            for f, v, r in tree:
                feat.append(f); value.append(v); right.append(r + base if r >= 0 else -1)
            tree_first.append(base + len(tree))
        forest_first.append(len(tree_first) - 1)
    iso_first = [0]
    for x, _ in calibrators:
        iso_first.append(iso_first[-1] + len(x))
    return {"version": np.int32(F.FORMAT_VERSION), "n_features": np.int32(n_features), "optimal_threshold": np.float64(optimal_threshold),
            "forest_first": np.asarray(forest_first, dtype=np.int32), "tree_first": np.asarray(tree_first, dtype=np.int32),
            "node_feature": np.asarray(feat, dtype=np.int32), "node_right": np.asarray(right, dtype=np.int32),
            "node_value": np.asarray(value, dtype=np.float64), "iso_first": np.asarray(iso_first, dtype=np.int32),
            "iso_x": np.asarray([v for x, _ in calibrators for v in x], dtype=np.float64),
            "iso_y": np.asarray([v for _, y in calibrators for v in y], dtype=np.float64)}


LEAF = -1
STUMP = [(0, 0.5, 2), (LEAF, 0.1, -1), (LEAF, 0.9, -1)]                       # x <= 0.5 -> 0.1, else 0.9
THR32 = float(np.float32(0.1))                                                # a threshold that is a float32, as scikit-learn's are
# four leaves by the value of feature 0: <= 1 -> 0.05, <= 2 -> 0.3, <= 3 -> 0.5, else 0.95
LADDER = [(0, 1.0, 2), (LEAF, 0.05, -1), (0, 2.0, 4), (LEAF, 0.3, -1), (0, 3.0, 6), (LEAF, 0.5, -1), (LEAF, 0.95, -1)]
KNOTS = ([0.1, 0.3, 0.7, 0.9], [0.0, 0.2, 0.6, 1.0])


def chain(depth: int):
    """A right-only chain: split i (node 2 i) sends x <= i to its leaf (value i / 100) and anything else on to split i + 1; past the last
    split lies the leaf 0.99, ``depth`` edges below the root."""
    tree = []
    for i in range(depth):
        tree += [(0, float(i), 2 * i + 2), (LEAF, i / 100.0, -1)]
    return tree + [(LEAF, 0.99, -1)]


def edge_cases():
    """(name, tables, X, the probabilities they must give - worked out by hand)."""
    above = THR32 + 1e-12                                                      # above the threshold as a double, ON it as a float32
    assert above > THR32 and float(np.float32(above)) == THR32
    return [
        ("a root that is a leaf", tables_of(2, [[[(LEAF, 0.25, -1)]]]), [[3.0, -1.0], [0.0, 0.0]], [0.25, 0.25]),
        ("x == threshold goes left", tables_of(1, [[STUMP]]), [[0.5], [np.nextafter(np.float32(0.5), np.float32(1))], [0.25]], [0.1, 0.9, 0.1]),
        ("the float32 rounding decides", tables_of(1, [[[(0, THR32, 2), (LEAF, 0.1, -1), (LEAF, 0.9, -1)]]]), [[above], [THR32 + 1e-7]], [0.1, 0.9]),
        ("a right-only chain of depth 40", tables_of(1, [[chain(40)]]), [[100.0], [17.5], [-1.0], [39.0], [39.5]], [0.99, 0.18, 0.0, 0.39, 0.99]),
        # forest means 0.05 (clipped below), 0.3 (a knot), 0.5 (between knots: 0.2 + (0.6 - 0.2) / (0.7 - 0.3) * (0.5 - 0.3)), 0.95 (clipped above)
        ("clip, knot and interpolation", tables_of(1, [[LADDER]], [KNOTS]), [[0.5], [1.5], [2.5], [3.5]],
         [0.0, 0.2, float(np.interp(0.5, *KNOTS)), 1.0]),
        ("a single-knot calibrator", tables_of(1, [[LADDER]], [([0.4], [0.33])]), [[0.5], [2.5], [3.5]], [0.33, 0.33, 0.33]),
        # two forests of two trees: means (0.1 + 0.05) / 2 and (0.05 + 0.1) / 2 at x = 0.25, each through its own calibrator, then averaged
        ("two forests, two calibrators", tables_of(1, [[STUMP, LADDER], [LADDER, STUMP]], [([0.0, 1.0], [0.0, 1.0]), ([0.0, 0.5], [0.5, 1.0])]),
         [[0.25]], [((0.1 + 0.05) / 2.0 + float(np.interp((0.05 + 0.1) / 2.0, [0.0, 0.5], [0.5, 1.0]))) / 2.0]),
    ]


def malformed():
    """(what is wrong, tables, a fragment of the message ``validate`` must give)."""
    def base():
        return tables_of(1, [[LADDER, LADDER]], [KNOTS])

    def mutate(key, index, value):
        t = base()
        t[key] = t[key].copy()
        t[key][index] = value
        return t
    no_knots = base()
    no_knots.update(iso_first=np.asarray([0, 0], dtype=np.int32), iso_x=np.zeros(0), iso_y=np.zeros(0))
    return [
        ("a child index <= its parent", mutate("node_right", 2, 2), "not greater than its parent"),
        ("a child outside its tree", mutate("node_right", 0, 8), "outside its tree"),
        ("feature >= n_features", mutate("node_feature", 0, 1), "below n_features"),
        ("a NaN threshold", mutate("node_value", 0, np.nan), "not finite"),
        ("a leaf value of 1.5", mutate("node_value", 1, 1.5), "outside [0, 1]"),
        ("non-increasing iso_x", mutate("iso_x", 2, 0.3), "strictly increasing"),
        ("an empty calibrator", no_knots, "empty calibrator"),
        ("depth 65", tables_of(1, [[chain(65)]]), "deeper than 64"),
    ]
