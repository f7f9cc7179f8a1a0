"""Batched on-GPU speech-to-text (rt_stt_transcribe_batch): the windows of all clips of a call are the rows of every launch, and a
clip's ids in a batch are the ids it gets alone - against transformers' Whisper (oracle/whisper.py) on the clips tests/test_stt_gpu.py
already holds the single-clip call to, against the single-clip call itself, and, below the ids, bit for bit on the encoder
states; then the provider's validation loop taking one transcription call per chunk.  The single-clip calls are the same path with
one row: "alone" is the clip as the only row, on buffers a larger call may have grown and written before."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from oracle import whisper as OW
from rho_tts_amd import _native
from rho_tts_amd import stt as S
from tests.test_oracle_whisper import boundary_clip, clip

pytestmark = pytest.mark.gpu

SR = 24000
EOS_SCALE = 6.0


@pytest.fixture(scope="module")
def ctx():
    c = _native.Context(0)
    yield c
    c.close()


def ragged_clips():
    edge = clip(2.0, SR, 5).copy()
    edge[-3:] = 0.9
    return [clip(1.3, SR, 3), clip(0.4, SR, 1), clip(2.6, SR, 2), np.zeros(int(0.7 * SR), dtype=np.float32), edge, clip(5.3, SR, 11),
            np.zeros(0, dtype=np.float32)]


def early_ending_state(cfg):
    """The seeded weights with the end-of-sequence row of the tied embedding / LM head scaled up (bf16-rounded): rows of a batch then
    end at different steps."""
    state = S.synthetic_state(cfg, 789)
    w = state["model.decoder.embed_tokens.weight"].clone()
    w[cfg.eos_id] = (w[cfg.eos_id].float() * EOS_SCALE).to(torch.bfloat16).to(w.dtype)
    state["model.decoder.embed_tokens.weight"] = w
    return state


@pytest.fixture(scope="module")
def tiny(ctx):
    cfg = S.tiny_test_config()
    state = early_ending_state(cfg)
    nat = S.NativeSTT(ctx, cfg, {k: v.cuda() for k, v in state.items()})
    yield cfg, state, nat
    nat.close()


def window_ids(model, cfg, x):
    """The oracle's ids of every 2-s window of a clip on its own."""
    win = cfg.chunk_seconds * SR
    return [OW.transcribe_windows(model, cfg, x[k * win:(k + 1) * win], SR) for k in range(max(1, -(-len(x) // win)))]


def test_ragged_batch_equals_the_oracle_and_the_single_call(tiny):
    """Seven clips, ten windows, rows ending at different steps (end-of-sequence row x 6.0: the oracle's window lengths come out
    [7] [12] [12, 12] [12] [12] [1, 1, 3] [12], smallest top-1 / top-2 logit gap 0.027 of the logits' standard deviation)."""
    cfg, state, nat = tiny
    clips = ragged_clips()
    model = OW.build(cfg, state)
    per_window = [window_ids(model, cfg, x) for x in clips]
    want = [OW.transcribe_windows(model, cfg, x, SR) for x in clips]
    assert want == [sum(w, []) for w in per_window] and sum(len(w) for w in per_window) == 10
    # (d) the fixture exercises the per-row end handling: a window that ends early, one that runs to the budget, and two windows of
    # one clip that end at different steps
    lens = [[len(i) for i in w] for w in per_window]
    print("window lengths", lens)
    flat = [n for w in lens for n in w]
    assert any(n < cfg.max_new_tokens for n in flat) and any(n == cfg.max_new_tokens for n in flat)
    assert any(len(set(w)) > 1 for w in lens if len(w) > 1)
    got = nat.transcribe_ids_batch(clips, SR)
    assert got == want                                                        # (a)
    assert got == [nat.transcribe_ids(x, SR) for x in clips]                  # (b)
    assert nat.transcribe_ids_batch(clips[::-1], SR) == want[::-1]            # (c)
    assert nat.transcribe_ids_batch(clips[:1], SR) + nat.transcribe_ids_batch(clips[1:], SR) == want
    assert nat.transcribe_ids_batch(clips, SR, max_tokens=15) == [w[:15] for w in want]      # (e)
    assert any(len(w) > 15 for w in want)


def test_more_windows_than_one_group(tiny):
    """Eleven 5.3-s clips of three windows each: 33 windows, one more than a group holds."""
    cfg, _, nat = tiny
    clips = [clip(5.3, SR, seed) for seed in range(11, 22)]
    got = nat.transcribe_ids_batch(clips, SR)
    assert got == [nat.transcribe_ids(x, SR) for x in clips] and all(got)
    # a cap the first windows fill (every window gives at least one id, the last clip's give 3, 3 and 12 on the oracle): the last clip's
    # third window is the second group's only window and is left out - the call ends without running an empty group; with a cap
    # of 12 it runs and is cut
    capped = nat.transcribe_ids_batch(clips, SR, max_tokens=2)
    assert capped == [nat.transcribe_ids(x, SR, max_tokens=2) for x in clips] == [g[:2] for g in got]
    assert len(capped[-1]) == 2 and len(got[-1]) > 12
    assert nat.transcribe_ids_batch(clips, SR, max_tokens=12) == [nat.transcribe_ids(x, SR, max_tokens=12) for x in clips]


def test_whisper_tiny_dimensions(ctx):
    """head_dim 64 x 6 heads, 1500 positions, the 51865-wide pick over three rows."""
    cfg = S.SttConfig(max_new_tokens=16)
    state = S.synthetic_state(cfg, 789)
    nat = S.NativeSTT(ctx, cfg, {k: v.cuda() for k, v in state.items()})
    try:
        clips = [clip(0.8, SR, 0), clip(3.3, SR, 3), clip(9.0, SR, 7)]
        got = nat.transcribe_ids_batch(clips, SR, max_tokens=12)
        assert got == [nat.transcribe_ids(x, SR, max_tokens=12) for x in clips]
        model = OW.build(cfg, state)
        assert got == [OW.transcribe_windows(model, cfg, x, SR, 12) for x in clips] and all(got)
    finally:
        nat.close()


def test_encoder_states_in_a_batch_are_the_bits_of_the_single_call(tiny):
    cfg, _, nat = tiny
    lib = nat.lib
    lib.rt_debug_stt_encode_batch.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.c_int32, C.c_int32, C.c_void_p]
    clips = ragged_clips()[:4]
    xs = [nat._pcm(x) for x in clips]
    out = torch.empty(len(xs), cfg.n_ctx, cfg.d_model, dtype=torch.float32, device=xs[0].device)
    ptrs = (C.c_void_p * len(xs))(*[x.data_ptr() for x in xs])
    lens = (C.c_int64 * len(xs))(*[x.numel() for x in xs])
    nat.ctx.check(lib.rt_debug_stt_encode_batch(nat.handle, ptrs, lens, len(xs), SR, C.c_void_p(out.data_ptr())), "rt_debug_stt_encode_batch")
    win = cfg.chunk_seconds * SR
    assert any(len(x) > win for x in clips)
    for i, x in enumerate(clips):
        assert torch.equal(out[i], nat.encode(x[:win], SR)), i   # (a clip longer than a window: its first window, cut as the transcription cuts it)


def single_stages(nat, x):
    ids, first = nat.transcribe_ids(x, SR, first_logits=True)
    return ids, first, nat.log_mel(x, SR), nat.encode(x, SR)


def test_a_grown_group_gives_a_single_clip_the_bits_of_a_fresh_handle(ctx, tiny):
    """One row over buffers sized and written by ten rows (seven ragged clips, two of them longer than a window): ids, the logits
    behind the prefix, log-mel and encoder states of a short clip equal those from a handle that has only ever seen that clip."""
    cfg, state, nat = tiny
    x = clip(0.9, SR, 4)
    fresh = S.NativeSTT(ctx, cfg, {k: v.cuda() for k, v in state.items()})
    try:
        want = single_stages(fresh, x)
    finally:
        fresh.close()
    clips = ragged_clips()
    assert len(clips) >= 3 and sum(nat.windows(len(c), SR) for c in clips) == 10 and any(nat.windows(len(c), SR) > 1 for c in clips)
    assert all(nat.transcribe_ids_batch(clips, SR))
    got = single_stages(nat, x)
    assert got[0] == want[0] and len(want[0]) > 0
    for name, g, w in zip(("first logits", "log-mel", "encoder states"), got[1:], want[1:]):
        assert torch.equal(g, w), name


def test_long_clip_at_a_non_native_rate(tiny):
    """log_mel / encode of a 3-s clip at 24 kHz on 2-s chunks keep the first chunk of the clip RESAMPLED WHOLE: the taps at the
    chunk's end see the samples behind it (tests/test_oracle_whisper.py shows that boundary_clip tells the two cuts apart by 0.37
    against the bound of 1e-4 that tests/test_stt_gpu.py holds the log-mel to).  Bit for bit the values the single-clip kernels
    gave before they were folded into the batched path (tests/golden/stt_boundary_clip.npz, recorded on an MI355X from the last
    build that had them)."""
    cfg, _, nat = tiny
    x = boundary_clip(cfg, SR)
    assert len(x) > cfg.chunk_seconds * SR
    mel, states = nat.log_mel(x, SR).cpu(), nat.encode(x, SR).cpu()
    err = float((mel - OW.log_mel(cfg, OW.resample(x, SR, cfg.sample_rate))).abs().max())
    print("log-mel against the oracle", err)
    assert err < 1e-4
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stt_boundary_clip.npz"))
    assert np.array_equal(mel.numpy(), g["log_mel"]) and np.array_equal(states.numpy(), g["states"])


def test_an_empty_clip_is_one_window_of_silence(tiny):
    cfg, state, nat = tiny
    empty = np.zeros(0, dtype=np.float32)
    ids = nat.transcribe_ids(empty, SR)
    assert ids == nat.transcribe_ids_batch([empty], SR)[0] == nat.transcribe_ids(np.zeros(cfg.chunk_seconds * SR, dtype=np.float32), SR)
    assert ids == OW.transcribe_windows(OW.build(cfg, state), cfg, empty, SR) and len(ids) > 0


def test_arguments(ctx):
    cfg = S.tiny_test_config()
    state = S.synthetic_state(cfg, 789)
    nat = S.NativeSTT(ctx, cfg, {k: v.cuda() for k, v in state.items()})
    x = clip(0.4, SR, 1)
    try:
        assert nat.transcribe_ids_batch([], SR) == []
        with pytest.raises(ValueError):
            nat.transcribe_ids_batch([x], 10)
        with pytest.raises(ValueError):
            nat.transcribe_ids_batch([x], SR, max_tokens=-1)
    finally:
        nat.close()
    with pytest.raises(ValueError):                  # a closed handle, as the single call refuses it
        nat.transcribe_ids(x, SR)
    with pytest.raises(ValueError):
        nat.transcribe_ids_batch([x], SR)


class CountingTranscriber:
    """WhisperTranscriber behind counters; `batch` can be hidden to take the per-segment path."""

    def __init__(self, tr, with_batch):
        self.tr, self.single_calls, self.batch_calls, self.sizes = tr, 0, 0, []
        if with_batch:
            self.batch = self._batch

    def __call__(self, audio, sr):
        assert audio.is_cuda
        self.single_calls += 1
        return self.tr(audio, sr)

    def _batch(self, audios, sr):
        assert all(a.is_cuda for a in audios)
        self.batch_calls += 1
        self.sizes.append(len(audios))
        return self.tr.batch(audios, sr)


def test_provider_validates_a_chunk_with_one_transcription_call(monkeypatch):
    """The validation loop on the device (tests/test_stt_gpu.py::test_validation_runs_on_the_device_without_a_file) with a
    transcriber that has `batch`: one call per generated chunk, none per segment, and what the per-segment path produces."""
    import tempfile
    from rho_tts_amd.provider import MI355XQwenTTS
    texts = ["A short sentence to validate.", "And another one.", "The third text.", "One more, the last."]

    def no_files(*a, **k):
        raise AssertionError("validation wrote a temporary file")
    monkeypatch.setattr(tempfile, "mkstemp", no_files)
    runs = []
    for with_batch in (True, False):
        t = MI355XQwenTTS(device="cuda", speaker="Vivian", model_path="x/CustomVoice-small", batch_size=4, max_iterations=2)
        try:
            eng = t._load_engine()
            tr = S.WhisperTranscriber(eng.ctx, synthetic=True, cfg=S.tiny_test_config())
            chunks = []
            gen = t._generate_chunk
            monkeypatch.setattr(t, "_generate_chunk", lambda *a, _g=gen, **k: (chunks.append(1), _g(*a, **k))[1])
            counting = CountingTranscriber(tr, with_batch)
            t.transcriber = counting
            t.drift_scorer = lambda audio, sr: 0.01
            t.drift_scorer.batch = lambda audios, sr: [0.01] * len(audios)
            t.text_similarity_threshold = 0.0                                # random weights transcribe nothing: every score is accepted
            res = t.generate(texts)
            assert res is not None and all(r is not None and r.audio.numel() > 0 for r in res)
            assert all(r.text_similarity is not None and r.drift_prob == 0.01 for r in res)
            runs.append((counting, len(chunks), [(r.text_similarity, r.audio.clone()) for r in res]))
            tr.close()
        finally:
            t.close()
    (b, b_chunks, b_res), (p, p_chunks, p_res) = runs
    assert b.batch_calls == b_chunks == p_chunks >= 1 and b.single_calls == 0 and sum(b.sizes) == p.single_calls >= len(texts)
    assert p.batch_calls == 0
    for (sim_b, audio_b), (sim_p, audio_p) in zip(b_res, p_res):
        assert sim_b == sim_p and torch.equal(audio_b, audio_p)
