#!/usr/bin/env python3
"""Drift classifier inference: DriftForest.predict (one native call: copy in, two launches, copy out, one stream synchronisation) for
1, 32 and 256 feature rows of the reference-shaped model - 286 features, 5 forests x 200 trees, depth 10, isotonic calibration -
beside scikit-learn's predict_proba for the same rows on the same host, when scikit-learn is importable there (the model is then
fitted here on random data and exported; otherwise the `full` model of tests/golden/forest_golden.npz is timed alone).  Every call
ends with its own stream synchronisation, so wall time around the call is the time of the call; the outputs are compared before
anything is timed.
    python tools/bench_forest.py [repeats]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch  # noqa: F401  (before the library: one HIP runtime per process)
from rho_tts_amd import _native
from rho_tts_amd import forest as F

REPEATS = int(sys.argv[1]) if len(sys.argv) > 1 else 51
WARMUP = 5
rng = np.random.default_rng(10)
model = None
try:
    from sklearn.calibration import CalibratedClassifierCV
    from sklearn.ensemble import RandomForestClassifier
    import sklearn
    Xt = rng.standard_normal((500, 286)).astype(np.float32)
    yt = (Xt[:, 0] + 0.7 * Xt[:, 1] + 0.8 * rng.standard_normal(500) > 0.3).astype(np.int64)
    model = CalibratedClassifierCV(RandomForestClassifier(n_estimators=200, max_depth=10, min_samples_leaf=10, min_samples_split=20,
                                                          random_state=42), method="isotonic", cv=5).fit(Xt, yt)
    tables = F.export_sklearn(model)
    print(f"model fitted here with scikit-learn {sklearn.__version__} (the trainer's hyper-parameters: n_jobs unset)")
except ImportError:
    z = np.load(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "forest_golden.npz"))
    tables = F.validate({k: z[f"full__{k}"] for k in F.KEYS})
    print("scikit-learn is not importable on this host: the golden `full` model, native call only")
print(f"{int(tables['n_features'])} features, {tables['forest_first'].shape[0] - 1} forests, {tables['tree_first'].shape[0] - 1} trees, "
      f"{tables['node_feature'].shape[0]} nodes, depth {F.tree_depth(tables)}", flush=True)


def median_ms(fn):
    for _ in range(WARMUP):
        fn()
    t = []
    for _ in range(REPEATS):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    t.sort()
    return t[len(t) // 2], t[0], t[-1]


ctx = _native.Context(0)
forest = F.DriftForest(ctx, tables)
for n in (1, 32, 256):
    X = rng.standard_normal((n, 286))
    got = forest.predict(X)
    line = f"{n:4d} rows: equal to predict_host: {bool(np.array_equal(got, F.predict_host(tables, X)))}"
    med, lo, hi = median_ms(lambda: forest.predict(X))
    line += f"   DriftForest.predict median {med:8.3f} ms (min {lo:.3f}, max {hi:.3f}, {REPEATS} calls)"
    if model is not None:
        want = model.predict_proba(X)[:, 1]
        smed, slo, shi = median_ms(lambda: model.predict_proba(X))
        line += f"   sklearn predict_proba median {smed:8.2f} ms (min {slo:.2f}, max {shi:.2f})   max |difference| {float(np.abs(got - want).max()):.2g}   ratio {smed / med:.0f}"
    print(line, flush=True)
forest.close()
ctx.close()
