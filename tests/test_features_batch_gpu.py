"""pYIN's back half on the GPU and the batched drift-feature call (csrc/features.hip k_feat_observe / k_feat_viterbi behind
rt_features_extract_batch; rho_tts_amd/features.py HandcraftedFeatures.batch) against the host functions that define them:
``viterbi_banded`` state for state, ``observation_log_probs`` in the probability domain, ``HandcraftedFeatures.__call__`` element
for element, and the CPU oracle (oracle/features.py) with the tolerances of tests/test_features_gpu.py."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import features as OF
from rho_tts_amd import _native
from rho_tts_amd import features as PF
from tests.test_features_batch_cpu import jump_log_obs, tie_log_obs
from tests.test_oracle_features import voiced

pytestmark = pytest.mark.gpu

SR = 24000
P = 601
PD, PI = C.POINTER(C.c_double), C.POINTER(C.c_int32)


@pytest.fixture(scope="module")
def ctx():
    c = _native.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ex(ctx):
    e = PF.HandcraftedFeatures(ctx)
    e.set_pitch_model()
    yield e
    e.close()


def gpu_viterbi(e, los):
    """State paths of the clips ``los`` (each [T][2 n_bins]) from ONE rt_debug_features_viterbi call."""
    n = len(los)
    stride = max(lo.shape[0] for lo in los)
    cat = np.ascontiguousarray(np.concatenate(los, axis=0), dtype=np.float64)
    nf = (C.c_int32 * n)(*[lo.shape[0] for lo in los])
    states = np.full((n, stride), -7, dtype=np.int32)
    e.ctx.check(e.lib.rt_debug_features_viterbi(e.handle, cat.ctypes.data_as(PD), nf, n, states.ctypes.data_as(PI), stride), "rt_debug_features_viterbi")
    for c, lo in enumerate(los):
        assert np.all(states[c, lo.shape[0]:] == -1)
    return [states[c, : lo.shape[0]].astype(np.int64) for c, lo in enumerate(los)]


def gpu_observe(e, cmnd):
    cmnd = np.ascontiguousarray(cmnd, dtype=np.float64)
    out = np.zeros((cmnd.shape[0], 2 * e.n_bins), dtype=np.float64)
    e.ctx.check(e.lib.rt_debug_features_observe(e.handle, cmnd.ctypes.data_as(PD), cmnd.shape[0], cmnd.shape[1], e.min_period, out.ctypes.data_as(PD)),
                "rt_debug_features_observe")
    return out


# ------------------------------------------------------------------------------------------------ 1. Viterbi, exact
def host_log_obs_of_a_voiced_clip():
    cm = OF.cmnd_frames(voiced(0.7, 16000, 300.0))
    assert cm.shape[0] == 22
    return PF.observation_log_probs(cm, OF.pitch_geometry()[0], P)


REAL = {
    "T1": lambda: np.random.default_rng(11).standard_normal((1, 2 * P)),
    "T2": lambda: np.random.default_rng(12).standard_normal((2, 2 * P)),
    "voiced": host_log_obs_of_a_voiced_clip,
    "jump": jump_log_obs,
    "ties": tie_log_obs,
    "all_equal": lambda: np.zeros((4, 2 * P)),
}


@pytest.mark.parametrize("case", list(REAL))
def test_viterbi_equals_the_host_at_the_real_geometry(ex, case):
    lo = REAL[case]()
    want = PF.viterbi_banded(lo, P)
    (got,) = gpu_viterbi(ex, [lo])
    assert np.array_equal(got, want), (got, want)
    if case == "jump":
        assert list(want[2:4]) == [500, 500]                              # 490 bins in one frame: only the outside-the-band rule gets there


@pytest.mark.parametrize("n_bins,hw,T", [(7, 2, 5), (5, 50, 4)])
def test_viterbi_equals_the_host_at_tiny_geometries(ctx, n_bins, hw, T):
    """Run-time geometry: a band of two bins either side, and a band wider than the state space."""
    e = PF.HandcraftedFeatures(ctx)
    try:
        e.set_pitch_model(PF.pitch_model(n_bins, hw))
        rng = np.random.default_rng(3)
        los = [rng.choice(np.array([0.0, -0.5, -1.0]), size=(T, 2 * n_bins)), rng.standard_normal((T, 2 * n_bins)), np.zeros((T, 2 * n_bins))]
        for lo, got in zip(los, gpu_viterbi(e, los)):
            assert np.array_equal(got, PF.viterbi_banded(lo, n_bins, hw))
    finally:
        e.close()


def test_viterbi_clips_of_different_lengths_in_one_call(ex):
    rng = np.random.default_rng(21)
    los = [rng.standard_normal((T, 2 * P)) for T in (1, 7, 3)]
    together = gpu_viterbi(ex, los)
    for lo, got in zip(los, together):
        (alone,) = gpu_viterbi(ex, [lo])
        assert np.array_equal(got, alone) and np.array_equal(got, PF.viterbi_banded(lo, P))


# ------------------------------------------------------------------------------------------------ 2. observation stage
def clip(kind):
    if kind == "voiced":
        return voiced(1.2, SR, 220.0, seed=220)
    if kind == "voiced300":
        return voiced(0.7, SR, 300.0, seed=300)
    if kind == "noise":
        return (0.1 * np.random.default_rng(5).standard_normal(int(0.5 * SR))).astype(np.float32)
    if kind == "silence":
        return np.zeros(int(0.6 * SR), dtype=np.float32)
    assert kind == "short"
    return voiced(0.05, SR, 200.0, seed=4)[-1000:]


@pytest.mark.parametrize("kind", ["voiced", "noise", "silence", "short"])
def test_observation_stage_matches_the_host(ex, kind):
    """Probability domain, 1e-12: sums of at most about a hundred non-negative float64 terms of a few ulp each.  (The log domain
    does not work: on a clean voiced frame the voiced mass is 1 +- an ulp, so the unvoiced probability is exactly 0 or ~1e-19.)"""
    _, cmnd, _ = ex.raw(torch.from_numpy(clip(kind)).cuda(), SR)
    want = PF.observation_log_probs(cmnd, ex.min_period, P)
    got = gpu_observe(ex, cmnd)
    assert got.shape == want.shape and np.all(np.isfinite(got))
    err = float(np.abs(np.exp(got) - np.exp(want)).max())
    print(f"{kind}: {cmnd.shape[0]} frames, max |exp(got) - exp(want)| = {err:.3e}")
    assert err <= 1e-12, err
    (states,) = gpu_viterbi(ex, [got])
    assert np.array_equal(states, PF.viterbi_banded(got, P))              # the device's Viterbi on the device's own log-obs


# ------------------------------------------------------------------------------------------------ 3. end to end
KINDS = ["voiced", "voiced300", "silence", "short", "noise"]


@pytest.fixture(scope="module")
def five(ex):
    xs = [torch.from_numpy(clip(k)).cuda() for k in KINDS]
    single = [ex(x, SR) for x in xs]
    host_states = []
    for x in xs:
        _, cmnd, _ = ex.raw(x, SR)
        host_states.append(PF.viterbi_banded(PF.observation_log_probs(cmnd, ex.min_period, P), P))
    return xs, single, host_states, ex.batch(xs, SR), ex.f0_states(xs, SR)


def test_batch_equals_the_single_clip_path(five):
    xs, single, host_states, batch, states = five
    assert batch.shape == (5, 30) and np.all(np.isfinite(batch))
    for c, kind in enumerate(KINDS):
        assert np.array_equal(batch[c, :26], single[c][:26]), kind             # the same kernels with the same arguments: the same bits
        assert np.array_equal(states[c], host_states[c]), (kind, states[c], host_states[c])
        assert batch[c, 26] == single[c][26] and batch[c, 27] == single[c][27], kind
        assert batch[c, 28] == single[c][28] and batch[c, 29] == single[c][29], kind    # the same LPC bits, the same np.roots
    assert batch[0, 26] > 0 and batch[2, 26] == 0.0 and batch[2, 28] == 0.0


def test_batch_matches_the_oracle(five):
    """The tolerances of tests/test_features_gpu.py: test_features_match_the_oracle for the voiced clips, test_feature_edge_cases for
    silence, the short clip and noise."""
    _, _, _, batch, _ = five
    for c, kind in enumerate(KINDS):
        got, ref = batch[c], OF.handcrafted_features(clip(kind), SR)
        assert ref.shape == (30,)
        if kind.startswith("voiced"):
            f0 = 220.0 if kind == "voiced" else 300.0
            assert float(np.abs(got[:26] - ref[:26]).max()) < 2e-3
            assert abs(got[26] - ref[26]) < 1e-6 * ref[26] and abs(got[27] - ref[27]) < 1e-6 * max(1.0, ref[27])
            assert abs(got[28] - ref[28]) < 0.5 and abs(got[29] - ref[29]) < 0.5
            assert abs(got[26] / (f0 * 22050 / 16000) - 1.0) < 0.02
        else:
            assert float(np.abs(got[:26] - ref[:26]).max()) < 5e-3
            assert abs(got[26] - ref[26]) <= 1e-6 * max(1.0, abs(ref[26])) and abs(got[27] - ref[27]) <= 1e-6 * max(1.0, abs(ref[27]))
            assert abs(got[28] - ref[28]) < 1.0 and abs(got[29] - ref[29]) < 1.0


def test_batch_of_one_equals_the_clip_inside_the_batch(ex, five):
    xs, _, _, batch, states = five
    for c in (0, 3):
        assert np.array_equal(ex.batch([xs[c]], SR)[0], batch[c])
        assert np.array_equal(ex.f0_states([xs[c]], SR)[0], states[c])


def test_scorer_batch_is_one_extractor_call(ex, five):
    xs, single, _, batch, _ = five
    seen = []

    def classifier(f):
        seen.append(f)
        return float(len(seen))
    score = PF.make_drift_scorer(ex, classifier, embed=lambda a, sr: np.zeros(256))
    assert score.batch(xs, SR) == [1.0, 2.0, 3.0, 4.0, 5.0]
    assert all(f.shape == (286,) and np.array_equal(f[256:], batch[c]) for c, f in enumerate(seen))


def test_bad_calls_are_refused_not_faulted(ctx, ex):
    with pytest.raises(ValueError):
        ex.batch([torch.zeros(1)], SR)
    x = torch.from_numpy(clip("short")).cuda()
    torch.cuda.synchronize()

    def native(e, n_samples, cap):
        ptrs, lens = (C.c_void_p * 1)(x.data_ptr()), (C.c_int64 * 1)(n_samples)
        stats, lpc, st, npf = np.zeros(26), np.zeros(PF.LPC_ORDER + 1), np.zeros(max(cap, 1), dtype=np.int32), (C.c_int32 * 1)()
        return e.lib.rt_features_extract_batch(e.handle, ptrs, lens, 1, SR, e.min_period, e.max_period, PF.LPC_ORDER, stats.ctypes.data_as(PD),
                                               lpc.ctypes.data_as(PD), st.ctypes.data_as(PI), cap, npf)
    assert native(ex, 1, 8) == _native.RT_ERR_INVALID                       # a clip below two samples
    assert native(ex, 1000, 1) == _native.RT_ERR_INVALID                    # two pitch frames, room for one
    assert native(ex, 1000, 2) == _native.RT_OK
    fresh = PF.HandcraftedFeatures(ctx)
    try:
        assert native(fresh, 1000, 8) == _native.RT_ERR_INVALID             # no pitch model yet: an error code, not a fault
        assert b"pitch model" in fresh.lib.rt_last_error(ctx.handle)
    finally:
        fresh.close()
