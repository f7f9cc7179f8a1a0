"""The batched drift-feature path without a GPU: the tables ``pitch_model`` uploads, the host Viterbi (whose expressions the tables
share) against the dense Viterbi of oracle/features.py on matrices that take the outside-the-band rule and the tie rules, and the
provider's chunk-level drift hook on the host mirror with a counting fake scorer."""
import numpy as np
import pytest
import torch

from oracle import features as OF
from rho_tts_amd import api
from rho_tts_amd import features as PF
from tests.test_pipeline_host import Fake

TINY = np.finfo(np.float64).tiny
P = OF.pitch_geometry()[3]


def jump_log_obs():
    """A one-hot pitch track jumping bin 10 -> 500 -> 10 over six frames: 490 bins is far outside the +-50 band."""
    obs = np.zeros((6, 2 * P))
    for t, b in enumerate([10, 10, 500, 500, 10, 10]):
        obs[t, b] = 1.0
    return np.log(obs + TINY)


def tie_log_obs(T=12, seed=7):
    """Log-obs drawn from three values: exact ties between candidates in every frame."""
    return np.random.default_rng(seed).choice(np.array([0.0, -0.5, -1.0]), size=(T, 2 * P))


def test_pitch_model_tables_have_the_stated_shapes():
    m = PF.pitch_model()
    assert (m["n_bins"], m["half_width"]) == (601, 50) == (P, PF.default_half_width())
    assert m["thresholds"].shape == m["beta"].shape == (PF.N_THRESHOLDS,) and m["thresholds"].dtype == m["beta"].dtype == np.float64
    assert m["log_trans"].shape == (2, 101, 601) and m["log_init"].shape == (1202,)
    assert m["log_trans"].flags.c_contiguous and m["log_trans"].dtype == np.float64
    assert m["log_tiny"] == float(np.log(TINY))
    assert np.array_equal(m["thresholds"], np.linspace(0.0, 1.0, 101)[1:]) and abs(float(m["beta"].sum()) - 1.0) < 1e-12
    # stay / switch: the centre of an interior column is log(1 / 51 * p + tiny); outside the state space the table holds log(tiny)
    assert m["log_trans"][0, 50, 300] == np.log(1.0 / 51.0 * 0.99 + TINY) and m["log_trans"][1, 50, 300] == np.log(1.0 / 51.0 * 0.01 + TINY)
    assert m["log_trans"][0, 0, 0] == m["log_tiny"] and np.all(m["log_init"][:601] == m["log_tiny"])
    t = PF.pitch_model(7, 2)
    assert t["log_trans"].shape == (2, 5, 7) and t["log_init"].shape == (14,)
    w = PF.pitch_model(5, 50)
    assert w["log_trans"].shape == (2, 101, 5)


@pytest.fixture(scope="module")
def dense():
    p_init = np.zeros(2 * P)
    p_init[P:] = 1.0 / P
    return OF.transition_matrix(), p_init


@pytest.mark.parametrize("make", [jump_log_obs, tie_log_obs])
def test_host_viterbi_equals_the_dense_viterbi(dense, make):
    """oracle.viterbi takes probabilities and logs them itself: both sides are handed the same log-obs by going through exp once."""
    trans, p_init = dense
    obs = np.exp(make())
    lo = np.log(obs + TINY)
    got = PF.viterbi_banded(lo, P)
    want = OF.viterbi(obs.T, trans, p_init)
    assert np.array_equal(got, want)
    if make is jump_log_obs:
        assert list(got[2:4]) == [500, 500] and got[1] % P == 10          # the jump is followed, through the outside-the-band rule


# ------------------------------------------------------------------------------------------------ the provider hook
class Scorer:
    """Drift by a script on the audio's length: a segment fails its first (length // 480) % 4 scorings, then passes (3: never, with
    three iterations - that segment ends as "best by drift")."""

    def __init__(self, with_batch=True, batch_raises=False):
        self.single_calls, self.batch_calls, self.seen = 0, 0, {}
        if with_batch:
            self.batch = self._batch_raises if batch_raises else self._batch

    def _one(self, audio):
        key = int(audio.numel())
        k = self.seen.get(key, 0)
        self.seen[key] = k + 1
        return 0.9 - 0.001 * k if k < (key // 480) % 4 else 0.05 + 1e-6 * (key % 97)

    def __call__(self, audio, sr):
        assert sr == 24000
        self.single_calls += 1
        return self._one(audio)

    def _batch(self, audios, sr):
        assert sr == 24000 and all(a is not None for a in audios)
        self.batch_calls += 1
        return [self._one(a) for a in audios]

    def _batch_raises(self, audios, sr):
        self.batch_calls += 1
        raise RuntimeError("synthetic batch failure")


class Counting(Fake):
    chunks = 0

    def _generate_chunk(self, segs, item_idx, token):
        self.chunks += 1
        return super()._generate_chunk(segs, item_idx, token)


TEXTS = ["Hello general test", "Something else entirely.", "A", "One more short one", "And the fifth text of the call", "Six"]


def run(scorer, bs=4, fail=None):
    t = Counting(batch_size=bs)
    t._max_chars_explicit = True
    t.max_iterations = 3
    t.drift_scorer = scorer
    t.transcriber = lambda audio, sr: None                       # (a failed transcription passes: the drift decides alone)
    if fail:
        t.fail_on = {fail}
    res = t._run_pipeline(list(TEXTS), api.CancellationToken(), None)
    return t, res


def same_results(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        if x is None or y is None:
            assert x is None and y is None
            continue
        assert torch.equal(x[0], y[0]) and x[1] == y[1] and x[2] == y[2]


@pytest.mark.parametrize("bs", [1, 4, 32])
def test_chunk_drifts_take_one_scorer_call_per_chunk(bs):
    plain, batched = Scorer(with_batch=False), Scorer()
    t0, r0 = run(plain, bs)
    t1, r1 = run(batched, bs)
    assert plain.single_calls > len(TEXTS) and plain.batch_calls == 0           # (the script made some segments retry)
    assert batched.single_calls == 0 and batched.batch_calls == t1.chunks == t0.chunks
    assert t1.calls == t0.calls                                                  # the same segments generated and retried, in the same order
    same_results(r0, r1)
    assert batched.seen == plain.seen
    assert any(r[2]["drift_prob"] > 0.5 for r in r1) and any(r[2]["drift_prob"] < 0.1 for r in r1)    # exhausted / accepted


def test_segment_without_audio_is_left_out_of_the_batch():
    plain, batched = Scorer(with_batch=False), Scorer()
    t0, r0 = run(plain, 4, fail="A")
    t1, r1 = run(batched, 4, fail="A")
    assert r1[2] is None and batched.single_calls == 0 and t1.calls == t0.calls
    same_results(r0, r1)


def test_failing_batch_falls_back_to_the_per_segment_call():
    plain, broken = Scorer(with_batch=False), Scorer(batch_raises=True)
    t0, r0 = run(plain)
    t1, r1 = run(broken)
    assert broken.batch_calls == t1.chunks and broken.single_calls == plain.single_calls
    assert t1.calls == t0.calls
    same_results(r0, r1)
