"""The drift classifier's tables on the host (rho_tts_amd/forest.py): the numpy walk that defines the kernels against scikit-learn's
own probabilities, the exporter, the validator, hand-built edge trees, the file format, and the scorer / provider plumbing with stubs."""
import numpy as np
import pytest

from rho_tts_amd import features as PF
from rho_tts_amd import forest as F
from tests import forest_cases as FC


# ------------------------------------------------------------------------------------------------ against scikit-learn
@pytest.mark.parametrize("name", FC.MODELS)
def test_host_walk_is_within_the_bound_of_sklearn(name):
    tables, X, proba, bound, host = FC.golden(name)
    assert X.shape == (64, int(tables["n_features"])) and host.shape == proba.shape == (64,)
    err = np.abs(host - proba)
    print(f"{name}: max |predict_host - sklearn| = {err.max():.3g}, bound {bound:.3g}")
    assert np.all(err <= bound), (name, float(err.max()), bound)
    assert np.all((host >= 0.0) & (host <= 1.0)) and float(host.max() - host.min()) > 0.2      # (not a constant)


def test_golden_models_have_the_issue_shapes():
    shapes = {n: (int(t["n_features"]), t["forest_first"].shape[0] - 1, int(t["forest_first"][1])) for n, (t, *_) in ((n, FC.golden(n)) for n in FC.MODELS)}
    assert shapes == {"small": (6, 5, 7), "hand30": (30, 5, 20), "full": (286, 5, 200)}
    assert F.tree_depth(FC.golden("full")[0]) == 10


def test_interpolation_is_np_interp_bit_for_bit():
    tables = FC.golden("small")[0]
    first = tables["iso_first"]
    m = np.concatenate([np.linspace(-0.1, 1.1, 20001), tables["iso_x"]])
    for c in range(first.shape[0] - 1):
        kx, ky = tables["iso_x"][first[c]: first[c + 1]], tables["iso_y"][first[c]: first[c + 1]]
        assert np.array_equal(F.calibrate_host(m, kx, ky), np.interp(np.clip(m, kx[0], kx[-1]), kx, ky))


def _fit(n_features=6, n_est=7, calibrated="isotonic", classes=2, seed=5):
    from sklearn.calibration import CalibratedClassifierCV
    from sklearn.ensemble import RandomForestClassifier
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((300, n_features)).astype(np.float32)
    score = X[:, 0] + 0.7 * X[:, 1] + 0.8 * rng.standard_normal(300)
    y = (score > 0.3).astype(np.int64) if classes == 2 else np.digitize(score, [-0.5, 0.5])
    rf = RandomForestClassifier(n_estimators=n_est, max_depth=6, min_samples_leaf=4, random_state=42)
    model = rf if calibrated is None else CalibratedClassifierCV(rf, method=calibrated, cv=5)
    return model.fit(X, y), rng.standard_normal((64, n_features))


def test_exporter_against_the_model_it_exports():
    pytest.importorskip("sklearn")
    model, X = _fit()
    tables = F.export_sklearn(model)
    assert F.validate(tables) is not tables and int(tables["n_features"]) == 6 and tables["forest_first"].tolist() == [0, 7, 14, 21, 28, 35]
    assert float(tables["optimal_threshold"]) == 0.18
    slope = max(float(np.max(np.diff(c.calibrators[0].y_thresholds_) / np.diff(c.calibrators[0].X_thresholds_)))
                for c in model.calibrated_classifiers_ if c.calibrators[0].X_thresholds_.shape[0] > 1)
    err = np.abs(F.predict_host(tables, X) - model.predict_proba(X)[:, 1])
    assert np.all(err <= FC.bound(7, slope)), (float(err.max()), FC.bound(7, slope))
    # the reference's metadata dict carries its threshold along
    meta = F.export_sklearn({"model": model, "optimal_threshold": 0.23, "feature_dim": 6})
    assert float(meta["optimal_threshold"]) == 0.23 and all(np.array_equal(meta[k], tables[k]) for k in F.KEYS if k != "optimal_threshold")


def test_exporter_takes_a_bare_forest():
    pytest.importorskip("sklearn")
    rf, X = _fit(calibrated=None)
    tables = F.export_sklearn(rf)
    assert tables["iso_first"].tolist() == [0] and tables["forest_first"].tolist() == [0, 7]
    err = np.abs(F.predict_host(tables, X) - rf.predict_proba(X)[:, 1])
    assert np.all(err <= FC.bound(7, 0.0)), float(err.max())


def test_exporter_refusals_name_the_reason():
    pytest.importorskip("sklearn")
    from sklearn.calibration import CalibratedClassifierCV
    from sklearn.linear_model import LogisticRegression
    with pytest.raises(ValueError, match="sigmoid"):
        F.export_sklearn(_fit(calibrated="sigmoid")[0])
    with pytest.raises(ValueError, match=r"classes are \[0, 1, 2\]"):
        F.export_sklearn(_fit(classes=3)[0])
    with pytest.raises(ValueError, match=r"classes are \[0, 1, 2\]"):
        F.export_sklearn(_fit(classes=3, calibrated=None)[0])
    rng = np.random.default_rng(0)
    X, y = rng.standard_normal((100, 3)), np.arange(100) % 2
    with pytest.raises(ValueError, match="LogisticRegression"):
        F.export_sklearn(CalibratedClassifierCV(LogisticRegression(), method="isotonic", cv=3).fit(X, y))
    with pytest.raises(ValueError, match="LogisticRegression"):
        F.export_sklearn({"model": LogisticRegression().fit(X, y)})
    with pytest.raises(ValueError, match="no 'model'"):
        F.export_sklearn({"optimal_threshold": 0.2})
    # a forest fitted on data with NaNs sends missing values where it learned to: such inputs are refused here, so is the model
    from sklearn.ensemble import RandomForestClassifier
    Xn = rng.standard_normal((300, 6)).astype(np.float32)
    yn = (Xn[:, 0] + 0.5 * rng.standard_normal(300) > 0).astype(np.int64)
    Xn[rng.random(Xn.shape) < 0.15] = np.nan
    with pytest.raises(ValueError, match="missing-value support"):
        F.export_sklearn(RandomForestClassifier(n_estimators=7, max_depth=6, random_state=0).fit(Xn, yn))


# ------------------------------------------------------------------------------------------------ the validator
@pytest.mark.parametrize("case", FC.malformed(), ids=lambda c: c[0])
def test_validate_refuses(case):
    _, tables, fragment = case
    with pytest.raises(ValueError) as e:
        F.validate(tables)
    assert fragment in str(e.value), str(e.value)


def test_validate_accepts_what_the_malformed_cases_start_from():
    t = F.validate(FC.tables_of(1, [[FC.LADDER, FC.LADDER]], [FC.KNOTS]))
    assert F.tree_depth(t) == 3
    assert F.tree_depth(F.validate(FC.tables_of(1, [[FC.chain(64)]]))) == 64              # the deepest tree the format takes
    with pytest.raises(ValueError, match="missing node_right"):
        F.validate({k: v for k, v in t.items() if k != "node_right"})
    with pytest.raises(ValueError, match="format version 2"):
        F.validate(dict(t, version=np.int32(2)))
    with pytest.raises(ValueError, match="calibrators for 2 forests"):
        F.validate(FC.tables_of(1, [[FC.STUMP], [FC.STUMP]], [FC.KNOTS]))
    with pytest.raises(ValueError, match="empty or descending"):
        F.validate(dict(t, tree_first=np.asarray([0, 7, 7, 14], dtype=np.int32), forest_first=np.asarray([0, 3], dtype=np.int32)))


# ------------------------------------------------------------------------------------------------ hand-built trees
@pytest.mark.parametrize("case", FC.edge_cases(), ids=lambda c: c[0])
def test_edge_trees(case):
    _, tables, X, want = case
    got = F.predict_host(F.validate(tables), np.asarray(X, dtype=np.float64))
    assert got.dtype == np.float64 and got.tolist() == list(want), (got.tolist(), want)


def test_inputs_the_trees_cannot_take_are_refused():
    tables = F.validate(FC.tables_of(2, [[[(FC.LEAF, 0.25, -1)]]]))
    for bad in (np.nan, np.inf, -np.inf, 3.5e38, -1e300):
        with pytest.raises(ValueError, match="NaN, infinite or beyond float32"):
            F.predict_host(tables, [[0.0, bad]])
    assert F.predict_host(tables, [[3.4e38, -3.4e38]]).tolist() == [0.25]
    assert F.predict_host(tables, np.zeros((0, 2))).shape == (0,)
    with pytest.raises(ValueError, match=r"\[n\]\[2\]"):
        F.predict_host(tables, np.zeros((3, 5)))


# ------------------------------------------------------------------------------------------------ the file
def test_save_load_round_trip(tmp_path):
    tables = FC.golden("small")[0]
    path = str(tmp_path / "small.npz")
    F.save(path, tables)
    back = F.load(path)
    assert set(back) == set(F.KEYS)
    for k in F.KEYS:
        a, b = np.asarray(tables[k]), np.asarray(back[k])
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), k
    # a file that needs unpickling is refused, not unpickled
    pickled = str(tmp_path / "pickled.npz")
    np.savez(pickled, **{**{k: tables[k] for k in F.KEYS}, "node_value": np.asarray(list(tables["node_value"]), dtype=object)})
    with pytest.raises(ValueError, match="(?i)pickle"):
        F.load(pickled)
    short = str(tmp_path / "short.npz")
    np.savez(short, **{k: tables[k] for k in F.KEYS if k != "iso_y"})
    with pytest.raises(ValueError, match="missing iso_y"):
        F.load(short)


# ------------------------------------------------------------------------------------------------ the scorer, with stubs
class StubExtractor:
    def __init__(self):
        self.calls = []

    def batch(self, audios, sample_rate):
        self.calls.append((len(audios), sample_rate))
        return np.arange(len(audios) * 30, dtype=np.float64).reshape(len(audios), 30)

    def __call__(self, audio, sample_rate):
        raise AssertionError("the forest scorer goes through batch()")


class StubForest:
    def __init__(self, n_features):
        self.n_features, self.calls = n_features, []

    def predict(self, X):
        self.calls.append(np.array(X))
        return np.linspace(0.1, 0.2, len(X))


def test_forest_scorer_makes_one_call_of_each_per_chunk():
    ex, forest = StubExtractor(), StubForest(30)
    score = PF.make_forest_scorer(ex, forest)
    out = score.batch(["a", "b", "c", "d", "e"], 24000)
    assert ex.calls == [(5, 24000)] and len(forest.calls) == 1 and forest.calls[0].shape == (5, 30)
    assert out == list(np.linspace(0.1, 0.2, 5)) and all(type(v) is float for v in out)
    assert score("a", 16000) == 0.1                                           # the single-clip form: the same path with one row
    assert ex.calls == [(5, 24000), (1, 16000)] and forest.calls[1].shape == (1, 30)
    assert score.batch([], 24000) == [] and len(forest.calls) == 2


def test_forest_scorer_places_the_embedding_first_and_checks_the_width():
    ex, forest = StubExtractor(), StubForest(32)
    seen = []

    def embed(audios, sample_rate):
        seen.append((len(audios), sample_rate))
        return np.full((len(audios), 2), 7.0)
    score = PF.make_forest_scorer(ex, forest, embed=embed)
    score.batch(["a", "b", "c"], 24000)
    X = forest.calls[0]
    assert seen == [(3, 24000)] and X.shape == (3, 32)
    assert np.all(X[:, :2] == 7.0) and np.array_equal(X[:, 2:], np.arange(90.0).reshape(3, 30))
    with pytest.raises(ValueError, match="286 features.*30"):
        PF.make_forest_scorer(ex, StubForest(286))                              # no embedding for the 256 dimensions in front
    with pytest.raises(ValueError, match="30 features"):
        PF.make_forest_scorer(ex, StubForest(30), embed=embed)
    embed.dim = 2
    with pytest.raises(ValueError, match="286 != 30 \\+ 2"):
        PF.make_forest_scorer(ex, StubForest(286), embed=embed)
    PF.make_forest_scorer(ex, StubForest(32), embed=embed)
    wrong = PF.make_forest_scorer(ex, StubForest(40), embed=lambda audios, sr: np.zeros((len(audios), 2)))
    with pytest.raises(ValueError, match=r"\[1\]\[10\]"):
        wrong("a", 24000)


# ------------------------------------------------------------------------------------------------ the provider's configuration
def _provider(**kw):
    from rho_tts_amd.provider import MI355XQwenTTS
    return MI355XQwenTTS(device="cuda", speaker="Vivian", model_path="x/CustomVoice-small", batch_size=4, max_iterations=2, **kw)


def test_provider_without_a_drift_model_is_unchanged():
    t = _provider()
    assert t.drift_scorer is None and t.drift_model_path is None and t.drift_embed is None and t.drift_optimal_threshold is None
    assert t.accent_drift_threshold == 0.17
    mine = lambda audio, sr: 0.5                                               # noqa: E731
    t.drift_scorer = mine
    assert t.drift_scorer is mine


def test_provider_refuses_a_configuration_that_cannot_score(tmp_path):
    t = _provider(drift_model_path=str(tmp_path / "drift_classifier.pkl"))
    with pytest.raises(ValueError, match="export_drift_classifier"):
        t.drift_scorer
    mine = lambda audio, sr: 0.5                                               # noqa: E731
    t.drift_scorer = mine                                                      # the caller's scorer wins: the path is not looked at
    assert t.drift_scorer is mine
    path = str(tmp_path / "full.npz")
    F.save(path, FC.golden("full")[0])
    t = _provider(drift_model_path=path)
    with pytest.raises(ValueError, match="drift_embed"):                       # 286 features, nobody to supply the first 256
        t.drift_scorer
    with pytest.raises(ValueError, match="drift_embed"):
        t._chunk_drifts([object()])                                            # ... and the validation loop does not swallow it
    path30 = str(tmp_path / "hand30.npz")
    F.save(path30, FC.golden("hand30")[0])
    t = _provider(drift_model_path=path30)
    t.drift_embed = lambda audios, sr: np.zeros((len(audios), 256))
    with pytest.raises(ValueError, match="drift_embed has no place"):
        t.drift_scorer
