"""The drift classifier on the device (csrc/forest.hip behind rho_tts_amd.forest.DriftForest): bit-equal to the host definition
``predict_host``, within the derived bound of scikit-learn's stored probabilities, independent of what shares the call, refusing bad
arguments on the host side of the call - and installed by the provider from ``drift_model_path``.  The models come from
tests/golden/forest_golden.npz: no scikit-learn here."""
import numpy as np
import pytest
import torch

from rho_tts_amd import _native
from rho_tts_amd import features as PF
from rho_tts_amd import forest as F
from tests import forest_cases as FC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = _native.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def forests(ctx):
    """One DriftForest per golden model, shared by the tests that only predict."""
    made = {name: F.DriftForest(ctx, FC.golden(name)[0]) for name in FC.MODELS}
    yield made
    for f in made.values():
        f.close()


def same_bits(a, b) -> bool:
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("name,n_rows", [("small", 1), ("small", 2), ("small", 33), ("small", 64), ("small", 65), ("small", 257), ("hand30", 64), ("full", 64)])
def test_parity_with_the_host_walk_and_sklearn(forests, name, n_rows):
    tables, X, proba, bound, host = FC.golden(name)
    rows = np.arange(n_rows) % 64                                              # sliced below 64 rows, repeated above
    got = forests[name].predict(X[rows])
    assert forests[name].n_features == X.shape[1] and forests[name].optimal_threshold == float(tables["optimal_threshold"])
    assert got.dtype == np.float64 and same_bits(got, host[rows]), float(np.abs(got - host[rows]).max())
    err = np.abs(got - proba[rows])
    print(f"{name} x {n_rows}: max |device - sklearn| = {err.max():.3g}, bound {bound:.3g}")
    assert np.all(err <= bound), (float(err.max()), bound)


@pytest.mark.parametrize("case", FC.edge_cases(), ids=lambda c: c[0])
def test_edge_trees(ctx, case):
    _, tables, X, want = case
    f = F.DriftForest(ctx, tables)
    try:
        got = f.predict(np.asarray(X, dtype=np.float64))
        assert same_bits(got, F.predict_host(F.validate(tables), X)) and got.tolist() == list(want)
    finally:
        f.close()


def test_a_row_does_not_depend_on_its_call(forests):
    for name in ("small", "full"):
        _, X, _, _, host = FC.golden(name)
        f = forests[name]
        alone, in64, in257 = f.predict(X[17:18]), f.predict(X), f.predict(X[np.arange(257) % 64])
        assert same_bits(alone[0], in64[17]) and same_bits(alone[0], host[17])
        assert all(same_bits(alone[0], in257[r]) for r in (17, 81, 145, 209))
        assert same_bits(in64, f.predict(X))                                   # two consecutive calls
        assert f.predict(np.zeros((0, X.shape[1]))).shape == (0,)              # no rows: nothing to do
        assert same_bits(f.predict(X[17]), alone)                              # a single row may come as a vector


def test_set_model_replaces_the_model(ctx):
    (full, Xf, _, _, host_f), (small, Xs, _, _, host_s) = FC.golden("full"), FC.golden("small")
    f = F.DriftForest(ctx, full)
    try:
        assert same_bits(f.predict(Xf), host_f)
        f.set_model(small)
        assert f.n_features == 6 and same_bits(f.predict(Xs), host_s)
        with pytest.raises(ValueError, match=r"\[n\]\[6\]"):
            f.predict(Xf)
    finally:
        f.close()


def test_refusals_happen_before_any_launch(ctx, tmp_path):
    """Argument checks on the host side of the call: each is RT_ERR_INVALID (a ValueError here), and a correct call follows each."""
    small, X, _, _, host = FC.golden("small")
    f = F.DriftForest(ctx)
    try:
        with pytest.raises(ValueError, match="no model set"):
            f.predict(X)
        out = np.zeros(1)
        pd = F.C.POINTER(F.C.c_double)
        assert f.lib.rt_forest_predict(f.handle, X.ctypes.data_as(pd), 1, out.ctypes.data_as(pd)) == _native.RT_ERR_INVALID
        # tables the native check refuses (handed over WITHOUT the Python validator): one child index out of range is enough
        for what, bad, _ in FC.malformed():
            assert F.set_model_raw(f.lib, f.handle, bad) == _native.RT_ERR_INVALID, what
        with pytest.raises(ValueError, match="no model set"):                  # nothing was uploaded
            f.predict(X)
        f.set_model(small)
        assert same_bits(f.predict(X), host)
        assert F.set_model_raw(f.lib, f.handle, FC.malformed()[1][1]) == _native.RT_ERR_INVALID
        assert same_bits(f.predict(X), host)                                   # a refused model leaves the one before it in place
        for bad in (np.nan, np.inf, -np.inf, 1e39):
            Xb = X.copy()
            Xb[63, 5] = bad
            with pytest.raises(ValueError, match="NaN, infinite or beyond float32"):
                f.predict(Xb)
            assert same_bits(f.predict(X), host)
        assert f.lib.rt_forest_predict(f.handle, X.ctypes.data_as(pd), -1, out.ctypes.data_as(pd)) == _native.RT_ERR_INVALID
        with pytest.raises(ValueError, match="strictly increasing"):           # ... and the Python validator stands in front of the upload
            f.set_model(FC.malformed()[5][1])
        assert same_bits(f.predict(X), host)
        path = str(tmp_path / "small.npz")
        F.save(path, small)
        f.set_model(path)
        assert same_bits(f.predict(X), host)
    finally:
        f.close()


def _provider(**kw):
    from rho_tts_amd.provider import MI355XQwenTTS
    return MI355XQwenTTS(device="cuda", speaker="Vivian", model_path="x/CustomVoice-small", batch_size=4, max_iterations=2, **kw)


TEXTS = ["A short sentence to validate.", "And another one."]


def test_the_provider_scores_drift_from_an_exported_file(tmp_path):
    """``drift_model_path`` alone: the provider builds extractor + forest + scorer on its engine's context, scores a validated chunk in
    one ``batch`` call, and the ``drift_prob`` of a one-segment text is the forest's probability for that segment's audio."""
    tables = FC.golden("hand30")[0]
    path = str(tmp_path / "hand30.npz")
    F.save(path, tables)
    t = _provider(drift_model_path=path, accent_drift_threshold=2.0)           # (the caller's threshold: every score passes, one attempt)
    try:
        eng = t._load_engine()
        scorer = t.drift_scorer
        assert scorer is t.drift_scorer and callable(scorer.batch)             # built once
        assert t.drift_optimal_threshold == float(tables["optimal_threshold"]) and t.accent_drift_threshold == 2.0
        chunks, inner = [], scorer.batch

        def batch(audios, sr):
            assert all(a.is_cuda for a in audios)
            chunks.append(([a.clone() for a in audios], sr))
            return inner(audios, sr)
        scorer.batch = batch
        res = t.generate(list(TEXTS))
        assert res is not None and all(r is not None and r.audio.numel() > 0 and r.segments_count == 1 for r in res)
        assert len(chunks) == 1 and len(chunks[0][0]) == 2                     # entered once for the validated chunk
        audios, sr = chunks[0]
        ex, forest = PF.HandcraftedFeatures(eng.ctx), F.DriftForest(eng.ctx, path)
        try:
            feats = ex.batch(audios, sr)
            want = forest.predict(feats)
        finally:
            forest.close()
            ex.close()
        assert same_bits(want, F.predict_host(tables, feats))
        assert [r.drift_prob for r in res] == [float(v) for v in want]
    finally:
        t.close()
    assert t._drift_native is None                                             # close() destroyed the handles it made


def test_the_provider_needs_drift_embed_for_a_wider_model(tmp_path):
    tables = FC.golden("full")[0]
    path = str(tmp_path / "full.npz")
    F.save(path, tables)
    t = _provider(drift_model_path=path, accent_drift_threshold=2.0)
    try:
        t._load_engine()
        with pytest.raises(ValueError, match="drift_embed"):
            t.generate(list(TEXTS))
        seen = []

        def embed(audios, sr):
            seen.append(len(audios))
            return np.zeros((len(audios), 256))
        t.drift_embed = embed
        res = t.generate(list(TEXTS))
        assert res is not None and seen == [2]
        assert all(r is not None and r.drift_prob is not None and 0.0 <= r.drift_prob <= 1.0 for r in res)
    finally:
        t.close()
