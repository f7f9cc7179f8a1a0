"""The provider's chunk-level transcription hook (``BatchedPipeline._chunk_texts``) without a GPU: the host mirror with the scripted
drift scorer of tests/test_features_batch_cpu.py and a scripted transcriber that counts its calls.  One ``transcriber.batch`` call per
chunk covers exactly the segments the per-segment order would transcribe - those whose voice check passed - and leaves the
accepted audio, the retries and the scores as they were."""
import pytest

from rho_tts_amd import api
from tests.test_features_batch_cpu import TEXTS, Counting, Scorer, same_results
from tests.test_pipeline_host import fake_wave

BY_LENGTH = {}
for _t in TEXTS:
    BY_LENGTH.setdefault(len(fake_wave(_t)), _t)       # (two texts share a length: the second one never matches its transcript)


class Transcriber:
    """Transcript by a script on the audio's length and on how often that length was heard: the first (length // 480) % 3 hearings
    give noise, which fails the text check; later ones give the first text of that length."""

    def __init__(self, with_batch=True, batch_raises=False, short=False):
        self.single_calls, self.batch_calls, self.seen, self.heard = 0, 0, {}, []
        self.batch_raises, self.short = batch_raises, short
        if with_batch:
            self.batch = self._batch

    def _one(self, audio):
        key = int(audio.numel())
        k = self.seen.get(key, 0)
        self.seen[key] = k + 1
        self.heard.append(key)
        return "zzzz qqqq" if k < (key // 480) % 3 else BY_LENGTH.get(key)

    def __call__(self, audio, sr):
        assert sr == 24000
        self.single_calls += 1
        return self._one(audio)

    def _batch(self, audios, sr):
        assert sr == 24000 and audios and all(a is not None for a in audios)
        self.batch_calls += 1
        if self.batch_raises:
            raise RuntimeError("synthetic batch failure")
        if self.short:
            return [None] * (len(audios) + 1)
        return [self._one(a) for a in audios]


class Pipeline(Counting):
    """Counts the chunks in which at least one segment passed the voice check - the chunks a batched transcription is due for - and
    the segments scored / passed."""
    voiced_chunks = scored = voiced = 0

    def _chunk_drifts(self, audios):
        drifts = super()._chunk_drifts(audios)
        if drifts is not None:
            ok = [d < self.accent_drift_threshold for d in drifts if d is not None]
            self.voiced_chunks += any(ok)
            self.scored += len(ok)
            self.voiced += sum(ok)
        return drifts


def run(transcriber, bs=4, fail=None, scorer=None):
    t = Pipeline(batch_size=bs)
    t._max_chars_explicit = True
    t.max_iterations = 3
    t.drift_scorer = scorer or Scorer()
    t.transcriber = transcriber
    if fail:
        t.fail_on = {fail}
    return t, t._run_pipeline(list(TEXTS), api.CancellationToken(), None)


@pytest.mark.parametrize("bs", [1, 4, 32])
def test_chunk_texts_take_one_transcriber_call_per_voiced_chunk(bs):
    plain, batched = Transcriber(with_batch=False), Transcriber()
    t0, r0 = run(plain, bs)
    t1, r1 = run(batched, bs)
    assert plain.batch_calls == 0 and plain.single_calls == len(plain.heard) > 0
    assert batched.single_calls == 0 and batched.batch_calls == t1.voiced_chunks == t0.voiced_chunks > 0
    assert t1.calls == t0.calls and t1.chunks == t0.chunks        # the same segments generated and retried, in the same order
    same_results(r0, r1)                                          # audio, segment counts and scores (drift_prob, text_similarity)
    assert sorted(batched.heard) == sorted(plain.heard)
    # the script did its work: a segment whose drift fails is not transcribed, and one failed the text check and was retried
    assert len(batched.heard) == t1.voiced == t0.voiced < t1.scored
    assert plain.seen[len(fake_wave("Six"))] == 2
    assert any(r[2].get("text_similarity", 0.0) >= 0.85 for r in r1) and any(r[2].get("text_similarity", 1.0) < 0.85 for r in r1)


@pytest.mark.parametrize("how", ["raises", "short"])
def test_failing_batch_falls_back_to_the_per_segment_call(how):
    plain, broken = Transcriber(with_batch=False), Transcriber(batch_raises=how == "raises", short=how == "short")
    t0, r0 = run(plain)
    t1, r1 = run(broken)
    assert broken.batch_calls == t1.voiced_chunks > 0 and broken.single_calls == plain.single_calls
    assert t1.calls == t0.calls and broken.heard == plain.heard
    same_results(r0, r1)


def test_scorer_without_batch_leaves_the_transcription_per_segment():
    plain, batched = Transcriber(with_batch=False), Transcriber()
    t0, r0 = run(plain, scorer=Scorer(with_batch=False))
    t1, r1 = run(batched, scorer=Scorer(with_batch=False))
    assert batched.batch_calls == 0 and batched.single_calls == plain.single_calls > 0
    assert t1.calls == t0.calls and batched.heard == plain.heard
    same_results(r0, r1)


def test_segment_without_audio_is_left_out_of_the_batch():
    plain, batched = Transcriber(with_batch=False), Transcriber()
    t0, r0 = run(plain, 4, fail="A")
    t1, r1 = run(batched, 4, fail="A")          # (_batch asserts that no absent audio reaches it)
    assert r1[2] is None and batched.single_calls == 0 and batched.batch_calls > 0 and t1.calls == t0.calls
    assert sorted(batched.heard) == sorted(plain.heard)
    same_results(r0, r1)


def test_no_drift_validator_at_all_transcribes_every_segment_with_audio():
    """No drift scorer and no file-based drift validator: the voice check passes by definition, every segment with audio is in the call."""
    plain, batched = Transcriber(with_batch=False), Transcriber()
    outs = []
    for tr in (plain, batched):
        t = Pipeline(batch_size=4)
        t._max_chars_explicit = True
        t.max_iterations = 3
        t.transcriber = tr
        outs.append((t, t._run_pipeline(list(TEXTS), api.CancellationToken(), None)))
    (t0, r0), (t1, r1) = outs
    assert batched.single_calls == 0 and batched.batch_calls == t1.chunks and sorted(batched.heard) == sorted(plain.heard)
    assert t1.calls == t0.calls
    same_results(r0, r1)
