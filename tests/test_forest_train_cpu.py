"""The drift classifier's trainer on the host (rho_tts_amd/forest_train.py): the split search pinned to scikit-learn's
DecisionTreeClassifier, the forest's quality held to scikit-learn's own seed-to-seed spread, the isotonic fit pinned to
IsotonicRegression, determinism and structure of the tables, the data splits, the errors, and ``train`` end to end on synthetic WAVs
with an injected feature callable (no GPU)."""
import json
import os
import wave

import numpy as np
import pytest

from rho_tts_amd import forest as F
from rho_tts_amd import forest_train as T


def ones(n):
    return np.ones((1, n), dtype=np.uint8)


# ------------------------------------------------------------------------------------------------ split search against scikit-learn
def _split_dataset(seed: int, n: int):
    rng = np.random.default_rng(1000 + seed)
    X = rng.standard_normal((n, 12))
    X[:, 5] = np.round(X[:, 5] * 4.0) / 4.0                                        # one column in quarter steps: many equal values
    y = (X[:, 2] + 0.6 * X[:, 7] + 0.7 * rng.standard_normal(n) > 0.2).astype(np.int64)   # two informative columns
    return X.astype(np.float32).astype(np.float64), y


def _score(x32col, y, thr, w0, w1):
    left = x32col.astype(np.float64) <= thr
    l0, l1 = w0 * float(np.sum(left & (y == 0))), w1 * float(np.sum(left & (y == 1)))
    r0, r1 = w0 * float(np.sum(~left & (y == 0))), w1 * float(np.sum(~left & (y == 1)))
    return (l0 * l0 + l1 * l1) / (l0 + l1) + (r0 * r0 + r1 * r1) / (r0 + r1)


def _all_scores(X32, y, w0, w1, msl):
    """Every valid boundary's (score, feature, threshold) under the module's formula, by brute force."""
    out = []
    n = X32.shape[0]
    for f in range(X32.shape[1]):
        v = np.sort(X32[:, f], kind="stable")
        for p in range(msl - 1, n - msl):
            if v[p] != v[p + 1]:
                thr = float(np.float64(v[p]) / 2.0 + np.float64(v[p + 1]) / 2.0)
                out.append((_score(X32[:, f], y, thr, w0, w1), f, thr))
    return out


def test_the_split_search_is_scikit_learns():
    from sklearn.tree import DecisionTreeClassifier
    w0, w1 = 2.5, 0.5                                                              # dyadic: scikit-learn's running sums are exact
    unique = 0
    for i in range(30):
        n = (40, 200, 1000)[i % 3]
        X, y = _split_dataset(i, n)
        X32 = X.astype(np.float32)
        t = T.fit_host(X, y, ones(n), T.FitParams(n_trees=1, max_depth=1, min_samples_leaf=10, min_samples_split=20, max_features=12,
                                                  w0=w0, w1=w1, bootstrap=False, seed=i))
        sk = DecisionTreeClassifier(max_depth=1, min_samples_leaf=10, min_samples_split=20, class_weight={0: w0, 1: w1}, random_state=0).fit(X32, y)
        assert t["node_feature"].shape[0] == 3 and sk.tree_.node_count == 3, (i, t["node_feature"], sk.tree_.node_count)
        ours_f, ours_thr = int(t["node_feature"][0]), float(t["node_value"][0])
        scores = _all_scores(X32, y, w0, w1, 10)
        best = max(s for s, _, _ in scores)
        assert _score(X32[:, ours_f], y, ours_thr, w0, w1) == best                 # ours is the best under the formula ...
        sk_f, sk_thr = int(sk.tree_.feature[0]), float(sk.tree_.threshold[0])
        assert _score(X32[:, sk_f], y, sk_thr, w0, w1) == best, (i, sk_f, sk_thr)  # ... and so is the partition scikit-learn chose
        if sum(1 for s, _, _ in scores if s == best) == 1:
            unique += 1
            assert (ours_f, ours_thr) == (sk_f, sk_thr), (i, ours_f, ours_thr, sk_f, sk_thr)
            want = sk.tree_.value[:, 0, 1]
            assert abs(float(t["node_value"][1]) - want[1]) <= 1e-12 and abs(float(t["node_value"][int(t["node_right"][0])]) - want[2]) <= 1e-12
    assert unique >= 25, unique


# ------------------------------------------------------------------------------------------------ forest quality
def _quality_data(seed, n):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, 60))
    score = X[:, 3] + 0.8 * X[:, 17] - 0.7 * X[:, 31] + 0.5 * X[:, 44] * X[:, 3] + 0.9 * rng.standard_normal(n)   # four informative columns
    return X, score


def test_the_forest_is_as_good_as_scikit_learns_own_spread():
    """n = 800, F = 60, class prior 0.35, the trainer's hyper-parameters and weights, 100 trees, Brier score on 3000 fresh rows: ours
    may exceed the worst of scikit-learn's random_state 0..9 by at most that set's max - min (the baseline's own seed-to-seed noise).
    Measured with scikit-learn 1.7.2: ours 0.1836; scikit-learn 0.1823 .. 0.1874 (worst + spread = 0.1925)."""
    from sklearn.ensemble import RandomForestClassifier
    Xa, sa = _quality_data(5, 3800)
    cut = np.quantile(sa, 0.65)
    ya = (sa > cut).astype(np.int64)                                               # prior of class 1: 0.35
    X, y, Xt, yt = Xa[:800], ya[:800], Xa[800:], ya[800:]
    w0, w1 = T.class_weights(y)
    ours = T.fit_host(X, y, ones(800), T.FitParams(n_trees=100, w0=w0, w1=w1, seed=42))
    brier = T.brier_score(F.predict_host(ours, Xt), yt)
    sk = []
    for rs in range(10):
        rf = RandomForestClassifier(n_estimators=100, max_depth=10, min_samples_leaf=10, min_samples_split=20, max_features="sqrt",
                                    random_state=rs, class_weight={0: w0, 1: w1}).fit(X.astype(np.float32), y)
        sk.append(T.brier_score(rf.predict_proba(Xt.astype(np.float32))[:, 1], yt))
    print(f"brier: ours {brier:.4f}; scikit-learn {min(sk):.4f} .. {max(sk):.4f}")
    assert brier <= max(sk) + (max(sk) - min(sk)), (brier, sk)


# ------------------------------------------------------------------------------------------------ isotonic
def _iso_cases():
    rng = np.random.default_rng(7)
    cases = []
    for n in (1, 2, 17, 500):
        x = np.round(rng.random(n) * 40.0) / 200.0 + rng.integers(0, 3, n) * 0.25  # forest-mean-like, many duplicates
        cases.append((f"n{n}", x, (rng.random(n) < np.clip(x, 0.05, 0.95)).astype(np.float64)))
    cases.append(("equal_x", np.full(9, 0.375), np.asarray([0, 1, 1, 0, 0, 1, 0, 0, 1], dtype=np.float64)))
    xs = np.linspace(0.05, 0.9, 12)
    cases.append(("monotone", xs, (xs > 0.5).astype(np.float64)))
    return cases


@pytest.mark.parametrize("case", _iso_cases(), ids=lambda c: c[0])
def test_isotonic_fit_is_scikit_learns(case):
    from sklearn.isotonic import IsotonicRegression
    _, x, y = case
    iso = IsotonicRegression(out_of_bounds="clip").fit(x, y)
    kx, ky = T.isotonic_fit(x, y)
    assert np.array_equal(kx, iso.X_thresholds_), (kx, iso.X_thresholds_)
    assert np.all(np.abs(ky - iso.y_thresholds_) <= 1e-12)
    probe = np.linspace(-0.1, 1.1, 57)
    assert np.all(np.abs(F.calibrate_host(probe, kx, ky) - iso.predict(probe)) <= 1e-12)


# ------------------------------------------------------------------------------------------------ determinism and structure
@pytest.fixture(scope="module")
def small():
    rng = np.random.default_rng(3)
    X = rng.standard_normal((150, 9))
    y = (X[:, 1] - X[:, 4] + 0.5 * rng.standard_normal(150) > 0).astype(np.int64)
    return X, y


def _nodes_of(t, first, last):
    k0, k1 = int(t["tree_first"][first]), int(t["tree_first"][last])
    r = t["node_right"][k0:k1].astype(np.int64)
    return t["node_feature"][k0:k1].tobytes(), np.where(r >= 0, r - k0, -1).tobytes(), t["node_value"][k0:k1].tobytes()


def test_same_inputs_same_tables_and_a_tree_does_not_depend_on_the_others(small):
    X, y = small
    p8 = T.FitParams(n_trees=8, min_samples_leaf=3, min_samples_split=6, w0=1.3, w1=0.7, seed=2 ** 40 + 5)
    a, b = T.fit_host(X, y, ones(150), p8), T.fit_host(X, y, ones(150), p8)
    assert all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in F.KEYS)
    p3 = T.FitParams(n_trees=3, min_samples_leaf=3, min_samples_split=6, w0=1.3, w1=0.7, seed=2 ** 40 + 5)
    c = T.fit_host(X, y, ones(150), p3)
    assert _nodes_of(c, 0, 3) == _nodes_of(a, 0, 3)
    other_seed = T.fit_host(X, y, ones(150), T.FitParams(n_trees=3, min_samples_leaf=3, min_samples_split=6, w0=1.3, w1=0.7, seed=6))
    assert _nodes_of(other_seed, 0, 3) != _nodes_of(c, 0, 3)
    assert F.tree_depth(a) <= 10 and F.validate(a)["iso_first"].shape[0] == 1


def test_another_forests_members_do_not_change_this_forest(small):
    X, y = small
    rng = np.random.default_rng(0)
    member = (rng.random((3, 150)) < 0.8).astype(np.uint8)
    p = T.FitParams(n_trees=4, min_samples_leaf=2, min_samples_split=4)
    a = T.fit_host(X, y, member, p)
    changed = member.copy()
    changed[1] = member[1][rng.permutation(150)]
    changed[2] = 1
    b = T.fit_host(X, y, changed, p)
    assert _nodes_of(a, 0, 4) == _nodes_of(b, 0, 4) and _nodes_of(a, 4, 8) != _nodes_of(b, 4, 8)
    for c in range(3):
        assert T.single_forest(a, c)["forest_first"].tolist() == [0, 4]            # validated bare tables of every forest
    with pytest.raises(ValueError, match="calibrators"):
        F.validate(a)                                                              # several forests serve only with their calibrators
    knots = [(np.asarray([0.2, 0.8]), np.asarray([0.0, 1.0]))] * 3
    assert T.with_calibrators(a, knots, 0.3)["optimal_threshold"] == 0.3


def test_leaf_rules(small):
    X, y = small
    one_class = T.fit_host(X, np.zeros(150, dtype=np.int64), ones(150), T.FitParams(n_trees=2))
    assert one_class["node_feature"].tolist() == [-1, -1] and one_class["node_value"].tolist() == [0.0, 0.0]
    stump = T.fit_host(X, y, ones(150), T.FitParams(n_trees=2, max_depth=0))
    assert stump["node_feature"].tolist() == [-1, -1]
    t = T.fit_host(X[:20], y[:20], ones(20), T.FitParams(n_trees=1, bootstrap=False, max_features=9))   # exactly 2 * min_samples_leaf rows
    assert t["node_feature"].shape[0] in (1, 3)
    if t["node_feature"].shape[0] == 3:
        assert int(np.sum(X[:20].astype(np.float32)[:, int(t["node_feature"][0])].astype(np.float64) <= t["node_value"][0])) == 10
    constant = np.zeros((150, 1))
    assert T.fit_host(constant, y, ones(150), T.FitParams(n_trees=1))["node_feature"].tolist() == [-1]
    assert T.tree_capacity(T.FitParams(), 640) == 127 and T.tree_capacity(T.FitParams(max_depth=3), 640) == 15
    assert T.tree_capacity(T.FitParams(), 5) == 1
    deep = T.fit_host(X, y, ones(150), T.FitParams(n_trees=3, max_depth=14, min_samples_leaf=1, min_samples_split=2))
    assert all(np.diff(deep["tree_first"]) <= T.tree_capacity(T.FitParams(max_depth=14, min_samples_leaf=1), 150))


def test_feature_draws_and_refusals(small):
    X, y = small
    for nf, k in ((1, 1), (9, 3), (9, 9), (286, 16)):
        d = T.feature_draws(123456789, nf, k)
        assert len(d) == k and len(set(d)) == k and all(0 <= f < nf for f in d)
    assert T.FitParams().features_per_node(286) == 16 and T.FitParams().features_per_node(1) == 1
    bad = X.copy()
    bad[3, 2] = np.nan
    with pytest.raises(ValueError, match="NaN"):
        T.fit_host(bad, y, ones(150), T.FitParams(n_trees=1))
    with pytest.raises(ValueError, match="0 and 1"):
        T.fit_host(X, y + 1, ones(150), T.FitParams(n_trees=1))
    with pytest.raises(ValueError, match="without member"):
        T.fit_host(X, y, np.zeros((1, 150), dtype=np.uint8), T.FitParams(n_trees=1))
    with pytest.raises(ValueError, match="at most"):
        T.fit_host(np.zeros((T.MAX_ROWS + 1, 1)), np.zeros(T.MAX_ROWS + 1), ones(T.MAX_ROWS + 1), T.FitParams(n_trees=1))
    with pytest.raises(ValueError, match="out of range"):
        T.fit_host(X, y, ones(150), T.FitParams(n_trees=1, max_depth=65))


def test_splits_are_stratified_and_cover_every_row():
    rng = np.random.default_rng(11)
    y = (rng.random(203) < 0.3).astype(np.int64)
    train, test = T.split_train_test(y, 42)
    assert np.array_equal(np.sort(np.concatenate([train, test])), np.arange(203))
    for cls in (0, 1):
        assert int(np.sum(y[test] == cls)) == int(np.floor(0.2 * np.sum(y == cls) + 0.5))
    assert np.array_equal(T.split_train_test(y, 42)[1], test) and not np.array_equal(T.split_train_test(y, 43)[1], test)
    fold = T.folds(y[train], 5)
    assert fold.shape == train.shape and set(fold.tolist()) == {0, 1, 2, 3, 4}
    for cls in (0, 1):
        counts = np.bincount(fold[y[train] == cls], minlength=5)
        assert counts.max() - counts.min() <= 1 and counts.sum() == int(np.sum(y[train] == cls))
    with pytest.raises(ValueError, match=r"class 1 \(bad\) has 3 rows in the training split, fewer than the 5 folds.*20 good and 3 bad"):
        T.folds(np.asarray([0] * 20 + [1] * 3), 5)
    assert T.class_weights(np.asarray([0] * 30 + [1] * 10)) == ((40 / 60) * 5.0, (40 / 20) * 1.0)
    thr, cost = T.threshold_sweep(np.asarray([0.1, 0.2, 0.8, 0.9]), np.asarray([0, 0, 1, 1]))
    assert abs(thr - 0.21) < 1e-9 and cost == 0.0                                  # the first threshold of the lowest cost (strict <)


# ------------------------------------------------------------------------------------------------ end to end on the host
def _write_wav(path, samples, sr=16000, channels=1):
    pcm = np.clip(np.round(samples * 32767.0), -32768, 32767).astype("<i2")
    if channels == 2:
        pcm = np.repeat(pcm, 2)
    with wave.open(path, "wb") as w:
        w.setnchannels(channels)
        w.setsampwidth(2)
        w.setframerate(sr)
        w.writeframes(pcm.tobytes())


def _toy_features(clips, sr):
    """Six numbers per clip: enough to tell a tone from noise."""
    rows = []
    for a in clips:
        a = np.asarray(a, dtype=np.float64)
        spec = np.abs(np.fft.rfft(a[:2048], 2048))
        rows.append([a.std(), np.abs(np.diff(a)).mean(), spec.max() / (spec.mean() + 1e-9), float(np.argmax(spec)), a.max(), float(sr) / 16000.0])
    return np.asarray(rows)


@pytest.fixture()
def dataset(tmp_path):
    rng = np.random.default_rng(21)
    os.makedirs(tmp_path / "good")
    os.makedirs(tmp_path / "bad")
    t = np.arange(4000) / 16000.0
    for i in range(30):
        _write_wav(str(tmp_path / "good" / f"g{i:02d}.wav"), 0.4 * np.sin(2 * np.pi * (150.0 + 10 * i) * t) + 0.01 * rng.standard_normal(4000),
                   channels=2 if i == 3 else 1)
        _write_wav(str(tmp_path / "bad" / f"b{i:02d}.wav"), 0.3 * rng.standard_normal(4000), sr=22050 if i == 4 else 16000)
    with open(tmp_path / "bad" / "broken.wav", "wb") as f:
        f.write(b"not a wav file")
    return tmp_path


def test_train_end_to_end_on_the_host(dataset, tmp_path):
    out = str(tmp_path / "model.npz")
    said = []
    assert T.train(str(dataset), output_path=out, progress_callback=said.append, features=_toy_features) == out
    tables = F.load(out)
    assert int(tables["n_features"]) == 6 and tables["forest_first"].tolist() == [0, 200, 400, 600, 800, 1000]
    assert tables["iso_first"].shape[0] == 6
    meta = json.load(open(str(tmp_path / "model.json")))
    for k in ("model_name", "optimal_threshold", "fn_cost", "fp_cost", "training_date", "class_distribution", "expected_cost", "brier_score",
              "n_features", "seed", "native_source_hash"):
        assert k in meta, k
    assert meta["class_distribution"] == {"good": 30, "bad": 30} and meta["optimal_threshold"] == float(tables["optimal_threshold"])
    clips = [T.read_wav(str(dataset / d / f))[0] for d, f in (("good", "g00.wav"), ("good", "g03.wav"), ("good", "g17.wav"), ("bad", "b00.wav"),
                                                                ("bad", "b11.wav"))]
    p = F.predict_host(tables, _toy_features(clips, 16000))
    assert p[:3].max() < p[3:].min(), p                                            # the two synthetic classes are separated
    assert "Loaded 30 files from good/" in said and "Loaded 30 files from bad/" in said and "Loaded 60 samples (30 good, 30 bad)" in said
    assert "Extracting: 10/61 (16%) — good/g09.wav" in said and "Training model (this may take a moment)..." in said
    assert any(s.startswith("Optimal threshold: ") for s in said) and said[-1].startswith(f"Model saved to {out} (threshold: ")


def test_train_errors(tmp_path):
    os.makedirs(tmp_path / "good")
    with pytest.raises(FileNotFoundError, match="Dataset folder not found: .*bad"):
        T.train(str(tmp_path), output_path=str(tmp_path / "m.npz"), features=_toy_features)
    os.makedirs(tmp_path / "bad")
    t = np.arange(4000) / 16000.0
    for i in range(2):
        _write_wav(str(tmp_path / "good" / f"g{i}.wav"), 0.4 * np.sin(2 * np.pi * 200.0 * t))
        _write_wav(str(tmp_path / "bad" / f"b{i}.wav"), 0.1 * np.cos(2 * np.pi * 900.0 * t))
    with pytest.raises(ValueError, match=r"Not enough samples to train a classifier \(found 4, need at least 5\)"):
        T.train(str(tmp_path), output_path=str(tmp_path / "m.npz"), features=_toy_features)
    for i in range(2, 12):
        _write_wav(str(tmp_path / "good" / f"g{i}.wav"), 0.4 * np.sin(2 * np.pi * 200.0 * t))
    with pytest.raises(ValueError, match=r"class 1 \(bad\) has 2 rows"):
        T.train(str(tmp_path), output_path=str(tmp_path / "m.npz"), features=_toy_features)
