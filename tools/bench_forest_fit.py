#!/usr/bin/env python3
"""Drift classifier training at the reference's shape - n = 1000 rows, 286 features, 5 forests x 200 trees, depth 10, the trainer's
hyper-parameters and fold masks: the native fit (forest_train.fit_device = one rt_forest_fit call: copy in, two launches, copy out,
one stream synchronisation), the host definition fit_host (once), and - when scikit-learn is importable on this host - its
CalibratedClassifierCV(RandomForestClassifier(...), isotonic, cv=5).fit with the trainer's settings on the same rows.  The device
tables are compared with the host's before anything is timed.
    python tools/bench_forest_fit.py [repeats]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch  # noqa: F401  (before the library: one HIP runtime per process)
from rho_tts_amd import _native
from rho_tts_amd import forest_train as T

REPEATS = int(sys.argv[1]) if len(sys.argv) > 1 else 11
N, NF = 1000, 286
rng = np.random.default_rng(26)
X = rng.standard_normal((N, NF)).astype(np.float32).astype(np.float64)
y = (X[:, 0] + 0.7 * X[:, 1] - 0.5 * X[:, 200] + 0.8 * rng.standard_normal(N) > 0.4).astype(np.int64)
fold = T.folds(y, 5)
member = np.stack([fold != c for c in range(5)]).astype(np.uint8)
w0, w1 = T.class_weights(y)
params = T.FitParams(w0=w0, w1=w1, seed=42)

ctx = _native.Context(0)
got = T.fit_device(ctx, X, y, member, params)
t0 = time.perf_counter()
want = T.fit_host(X, y, member, params)
host_s = time.perf_counter() - t0
keys = ("tree_first", "node_feature", "node_right", "node_value")
print(f"{N} rows x {NF} features, 5 x {params.n_trees} trees, {got['node_feature'].shape[0]} nodes; "
      f"device tables equal to fit_host: {all(got[k].tobytes() == want[k].tobytes() for k in keys)}", flush=True)
t = []
for _ in range(REPEATS):
    t0 = time.perf_counter()
    T.fit_raw(ctx, X, y, member, params)
    t.append((time.perf_counter() - t0) * 1e3)
t.sort()
print(f"rt_forest_fit      median {t[len(t) // 2]:9.2f} ms (min {t[0]:.2f}, max {t[-1]:.2f}, {REPEATS} calls)")
print(f"fit_host (numpy)          {host_s * 1e3:9.0f} ms (one call)")
try:
    import sklearn
    from sklearn.calibration import CalibratedClassifierCV
    from sklearn.ensemble import RandomForestClassifier
    s = []
    for _ in range(3):
        model = CalibratedClassifierCV(RandomForestClassifier(n_estimators=200, max_depth=10, min_samples_leaf=10, min_samples_split=20,
                                                              max_features="sqrt", random_state=42, class_weight={0: w0, 1: w1}),
                                       method="isotonic", cv=5)
        t0 = time.perf_counter()
        model.fit(X, y)
        s.append((time.perf_counter() - t0) * 1e3)
    s.sort()
    print(f"scikit-learn {sklearn.__version__} CalibratedClassifierCV.fit (n_jobs unset) median {s[1]:9.0f} ms (min {s[0]:.0f}, max {s[-1]:.0f}, 3 calls)   "
          f"ratio to rt_forest_fit {s[1] / t[len(t) // 2]:.0f}")
except ImportError:
    print("scikit-learn is not importable on this host: native and host fits only")
ctx.close()
