"""Fitting the drift classifier's forests on the device (csrc/forest_fit.hip behind rho_tts_amd.forest_train.fit_device): the tables
of ``rt_forest_fit`` equal ``fit_host``'s bit for bit - tree_first, node_feature, node_right, node_value - at the smallest shapes at
which the kernels can go wrong; a tree does not depend on the others of its call; bad arguments are refused with their status; and
``train`` runs through a provider's context and installs the model it wrote."""
import os
import wave

import numpy as np
import pytest

from rho_tts_amd import _native
from rho_tts_amd import forest as F
from rho_tts_amd import forest_train as T

pytestmark = pytest.mark.gpu

TABLE_KEYS = ("forest_first", "tree_first", "node_feature", "node_right", "node_value")


@pytest.fixture(scope="module")
def ctx():
    c = _native.Context(0)
    yield c
    c.close()


def data(n, nf, seed=0):
    """Two informative columns where there is room; column 1 constant and column 2 of 4 distinct values when nf >= 4."""
    rng = np.random.default_rng(100 + seed)
    X = rng.standard_normal((n, nf))
    s = X[:, 0] + (0.7 * X[:, nf - 1] if nf > 1 else 0.0) + 0.6 * rng.standard_normal(n)
    if nf >= 4:
        X[:, 1] = 0.25
        X[:, 2] = rng.integers(0, 4, n).astype(np.float64) - 1.5
        s = s + 0.8 * X[:, 2]
    return X, (s > 0.3).astype(np.int64)


def fold_masks(y, k=5):
    return np.stack([T.folds(y, k) != c for c in range(k)]).astype(np.uint8)


def same_tables(a, b):
    return [k for k in TABLE_KEYS if np.asarray(a[k]).dtype != np.asarray(b[k]).dtype or np.asarray(a[k]).tobytes() != np.asarray(b[k]).tobytes()]


P = T.FitParams
SMALL = dict(min_samples_leaf=3, min_samples_split=6)
# (id, n, F, forests, params)
CASES = [
    ("n45", 45, 7, 1, P(n_trees=3, w0=1.7, w1=0.6, **SMALL)),
    ("n64", 64, 7, 1, P(n_trees=3, w0=1.7, w1=0.6, **SMALL)),
    ("n65", 65, 7, 1, P(n_trees=3, w0=1.7, w1=0.6, **SMALL)),
    ("n257", 257, 7, 1, P(n_trees=3, w0=1.7, w1=0.6, **SMALL)),
    ("n1000_reference_shape", 1000, 286, 1, P(n_trees=3, w0=3.1, w1=0.9)),
    ("n1000_five_folds", 1000, 30, 5, P(n_trees=3, w0=3.1, w1=0.9)),
    ("f1", 257, 1, 1, P(n_trees=3, **SMALL)),
    ("f7_all_features", 257, 7, 1, P(n_trees=3, max_features=7, **SMALL)),
    ("f30_one_feature", 257, 30, 1, P(n_trees=3, max_features=1, **SMALL)),
    ("f286_sqrt", 65, 286, 1, P(n_trees=1, **SMALL)),
    ("trees8_five_folds", 257, 7, 5, P(n_trees=8, w0=0.9, w1=2.3, **SMALL)),
    ("no_bootstrap", 257, 7, 1, P(n_trees=3, bootstrap=False, max_features=7, **SMALL)),
    ("no_bootstrap_five_folds", 65, 7, 5, P(n_trees=1, bootstrap=False, **SMALL)),
    ("depth0", 257, 7, 1, P(n_trees=3, max_depth=0)),
    ("depth1", 257, 7, 1, P(n_trees=3, max_depth=1)),
    ("depth10_leaf1", 257, 7, 1, P(n_trees=3, max_depth=10, min_samples_leaf=1, min_samples_split=2, w0=1.1, w1=0.7)),
    ("depth14_leaf1", 1000, 7, 1, P(n_trees=3, max_depth=14, min_samples_leaf=1, min_samples_split=2, w0=1.1, w1=0.7)),
    ("seed_high_word", 65, 7, 1, P(n_trees=3, seed=2 ** 63 + 12345, **SMALL)),
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0])
def test_device_tables_equal_the_host_definition(ctx, case):
    name, n, nf, n_forests, params = case
    X, y = data(n, nf, seed=len(name))
    member = np.ones((1, n), dtype=np.uint8) if n_forests == 1 else fold_masks(y, n_forests)
    want = T.fit_host(X, y, member, params)
    got = T.fit_device(ctx, X, y, member, params)
    assert same_tables(got, want) == [], (name, got["tree_first"][:6], want["tree_first"][:6])
    sizes = np.diff(want["tree_first"])
    print(f"{name}: {sizes.sum()} nodes, trees of {sizes.min()} .. {sizes.max()}, depth {max(F.tree_depth(T.single_forest(want, c)) for c in range(n_forests))}")
    if name.startswith("depth1") and "leaf1" in name:
        assert sizes.max() > 31                                                     # deep, many-node trees indeed
    assert same_tables(T.fit_device(ctx, X, y, member, params), want) == []        # a second call: the workspaces are reused


def test_one_class_and_exactly_two_leaves_of_rows(ctx):
    X, y = data(65, 7)
    got = T.fit_device(ctx, X, np.ones(65, dtype=np.int64), np.ones((1, 65), dtype=np.uint8), P(n_trees=3, **SMALL))
    assert got["node_feature"].tolist() == [-1, -1, -1] and got["node_value"].tolist() == [1.0, 1.0, 1.0]
    member = np.zeros((2, 65), dtype=np.uint8)                                     # forest 0 sees one class only, forest 1 both
    member[0, y == 0] = 1
    member[1] = 1
    p = P(n_trees=2, **SMALL)
    assert same_tables(T.fit_device(ctx, X, y, member, p), T.fit_host(X, y, member, p)) == []
    X20, y20 = X[:20], np.asarray([0, 1] * 10)
    p = P(n_trees=1, bootstrap=False, max_features=7)                              # 20 rows = 2 * min_samples_leaf: one boundary at most
    want = T.fit_host(X20, y20, np.ones((1, 20), dtype=np.uint8), p)
    assert want["node_feature"].shape[0] == 3 and same_tables(T.fit_device(ctx, X20, y20, np.ones((1, 20), dtype=np.uint8), p), want) == []


def test_a_tree_does_not_depend_on_the_other_trees_of_its_call(ctx):
    X, y = data(257, 7)
    member = np.ones((1, 257), dtype=np.uint8)
    t3, t8 = (T.fit_device(ctx, X, y, member, P(n_trees=k, w0=1.7, w1=0.6, **SMALL)) for k in (3, 8))
    k = int(t3["tree_first"][-1])
    assert np.array_equal(t3["tree_first"], t8["tree_first"][:4])
    assert all(t3[key].tobytes() == t8[key][:k].tobytes() for key in ("node_feature", "node_right", "node_value"))


def test_refusals(ctx):
    X, y = data(65, 7)
    member = np.ones((1, 65), dtype=np.uint8)
    p = P(n_trees=2, **SMALL)
    bad = X.copy()
    bad[5, 3] = np.inf
    assert T.fit_raw(ctx, bad, y, member, p)[0] == _native.RT_ERR_INVALID
    assert T.fit_raw(ctx, X, y + 1, member, p)[0] == _native.RT_ERR_INVALID
    assert T.fit_raw(ctx, X, y, np.zeros((1, 65), dtype=np.uint8), p)[0] == _native.RT_ERR_INVALID
    assert T.fit_raw(ctx, X, y, member, P(n_trees=2, max_depth=65))[0] == _native.RT_ERR_LENGTH
    assert T.fit_raw(ctx, X, y, member, p, node_cap=5)[0] == _native.RT_ERR_LENGTH
    assert T.fit_raw(ctx, X, y, member, P(n_trees=2, w0=0.0))[0] == _native.RT_ERR_INVALID
    n_big = T.MAX_ROWS + 1
    assert T.fit_raw(ctx, np.zeros((n_big, 1)), np.zeros(n_big), np.ones((1, n_big), dtype=np.uint8), P(n_trees=1), node_cap=8)[0] == _native.RT_ERR_LENGTH
    assert T.fit_raw(ctx, np.zeros((4, T.MAX_FEATURES + 1)), np.zeros(4), np.ones((1, 4), dtype=np.uint8), P(n_trees=1), node_cap=8)[0] == _native.RT_ERR_LENGTH
    with pytest.raises(ValueError, match="NaN, infinite"):
        ctx.check(T.fit_raw(ctx, bad, y, member, p)[0], "rt_forest_fit")
    rc, tree_first, feat, right, value = T.fit_raw(ctx, X, y, member, p)           # the handle is as usable as before
    assert rc == 0 and tree_first[-1] == feat.shape[0] > 0


def _write_wav(path, samples, sr=16000):
    with wave.open(path, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(sr)
        w.writeframes(np.clip(np.round(samples * 32767.0), -32768, 32767).astype("<i2").tobytes())


def test_train_through_a_provider_installs_the_model(tmp_path):
    from rho_tts_amd.features import HandcraftedFeatures
    from rho_tts_amd.provider import MI355XQwenTTS
    rng = np.random.default_rng(2)
    os.makedirs(tmp_path / "good")
    os.makedirs(tmp_path / "bad")
    t = np.arange(8000) / 16000.0                                                  # half a second
    for i in range(20):
        tone = 0.4 * np.sin(2 * np.pi * (140.0 + 9 * i) * t) + 0.1 * np.sin(2 * np.pi * (420.0 + 27 * i) * t) + 0.005 * rng.standard_normal(8000)
        _write_wav(str(tmp_path / "good" / f"g{i:02d}.wav"), tone)
        _write_wav(str(tmp_path / "bad" / f"b{i:02d}.wav"), 0.25 * rng.standard_normal(8000))
    out = str(tmp_path / "voice_classifier.npz")
    tts = MI355XQwenTTS(device="cuda", speaker="Vivian", model_path="x/CustomVoice-small", batch_size=4, max_iterations=2)
    try:
        assert tts.drift_scorer is None
        said = []
        assert tts.train_drift_classifier(str(tmp_path), output_path=out, progress_callback=said.append) == out
        assert tts.drift_model_path == out and os.path.exists(str(tmp_path / "voice_classifier.json"))
        assert "Loaded 40 samples (20 good, 20 bad)" in said and said[-1].startswith("Model saved to ")
        tables = F.load(out)
        assert int(tables["n_features"]) == 30 and tables["forest_first"].tolist() == [0, 200, 400, 600, 800, 1000] and tables["iso_first"].shape[0] == 6
        clips = [T.read_wav(str(tmp_path / d / f"{d[0]}{i:02d}.wav"))[0] for d in ("good", "bad") for i in range(20)]
        scorer = tts.drift_scorer                                                   # built from the new file at first use
        assert scorer is not None and tts.drift_optimal_threshold == float(tables["optimal_threshold"])
        ex = HandcraftedFeatures(tts._native_ctx())
        forest = F.DriftForest(tts._native_ctx(), out)
        try:
            rows = np.concatenate([ex.batch(clips[:32], 16000), ex.batch(clips[32:], 16000)])
            host = F.predict_host(tables, rows)
            assert forest.predict(rows).tobytes() == host.tobytes()
        finally:
            forest.close()
            ex.close()
        assert scorer.batch(clips[:32], 16000) + scorer.batch(clips[32:], 16000) == [float(v) for v in host]
        assert float(np.mean(host[:20])) < float(np.mean(host[20:]))               # tones against noise: the classes come apart
        # the forests of the file are what the host definition fits on the same rows: the device trained this model
        rows_y = np.asarray([0] * 20 + [1] * 20)
        again, _ = T.fit_classifier(rows, rows_y, seed=42)
        assert same_tables(again, tables) == [] and again["iso_x"].tobytes() == tables["iso_x"].tobytes()
    finally:
        tts.close()
