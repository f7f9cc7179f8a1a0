"""The GE2E speaker encoder on the device (csrc/speaker.hip behind rho_tts_amd.speaker.SpeakerEmbedder) against its float64 oracle
(tests/speaker_embed_ref.py), stage by stage - with seeded weights the final vector alone would hide a broken front end - then end to
end, with voice flags, assembled into the 286-d drift vector by the provider, and as the provider's speaker similarity.
Parity with resemblyzer is unpinned; the bounds are the issue's: 1e-6 max(mel) for the mel, 1e-4 for embeddings."""
import functools
import wave

import numpy as np
import pytest
import torch

from oracle import whisper as OW
from rho_tts_amd import _native
from rho_tts_amd import features as PF
from rho_tts_amd import forest as F
from rho_tts_amd import speaker as S
from tests import forest_cases as FC
from tests import speaker_embed_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = _native.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def emb(ctx):
    e = S.SpeakerEmbedder(ctx, synthetic=True)
    yield e
    e.close()


def voice(n: int, seed: int, amp: float = 0.1) -> np.ndarray:
    """A seeded, voice-like float32 clip: harmonics of a wandering pitch under a syllable-rate envelope, plus noise."""
    rng = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64) / 16000.0
    f0 = 110.0 + 40.0 * rng.random() + 15.0 * np.sin(2 * np.pi * (0.7 + rng.random()) * t)
    ph = 2 * np.pi * np.cumsum(f0) / 16000.0
    x = sum(rng.random() / (k + 1) * np.sin((k + 1) * ph + rng.random()) for k in range(8))
    x = x * (0.55 + 0.45 * np.sin(2 * np.pi * 3.1 * t + rng.random())) + 0.05 * rng.standard_normal(n)
    return (amp * x / np.abs(x).max()).astype(np.float32)


@functools.lru_cache(maxsize=None)
def e2e_case():
    """(clips, their rates' common value, 16-kHz versions, oracle embeddings, oracle partial counts) - computed once, read-only."""
    clips = [voice(8000, 1), voice(37000, 2), voice(217600, 3)]
    want = [R.embed(R.state(), x) for x in clips]
    return clips, np.stack([w[0] for w in want]), [w[1] for w in want]


def same_bits(a, b) -> bool:
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ------------------------------------------------------------------------------------------------ 1. mel
@pytest.mark.parametrize("amp", [0.01, 0.5])
def test_mel_of_the_preprocessed_clip(emb, amp):
    x = voice(8000, 7, amp)
    y = R.preprocess(x)
    scaled = not np.array_equal(y, x)
    assert scaled == (amp == 0.01)                                             # the quiet clip is brought up, the loud one left alone
    _, n_pad = S.partial_slices(len(y))
    want = R.mel(np.concatenate([y, np.zeros(n_pad - len(y), dtype=np.float32)]))
    got, n16 = emb.debug_mel(x, 16000)
    assert n16 == len(y) == 8000 and got.shape == want.shape == (161, 40) and got.dtype == np.float32
    err, top = float(np.abs(got - want).max()), float(want.max())
    print(f"mel amp {amp}: max |device - oracle| = {err:.3g}, max(mel) = {top:.3g}, bound {1e-6 * top:.3g}")
    assert err <= 1e-6 * top


# ------------------------------------------------------------------------------------------------ 2. the network
def test_lstm_against_the_float64_oracle(emb):
    rng = np.random.default_rng(17)
    parts = rng.standard_normal((17, 160, 40)).astype(np.float32)              # O(1) inputs: the gates leave their linear range
    want = R.partial_embeds(R.state(), parts.astype(np.float64))
    t32 = R.partial_embeds(R.state(), parts, torch.float32)
    got17, got1 = emb.debug_lstm(parts), emb.debug_lstm(parts[:1])
    err17, err1, err_t = float(np.abs(got17 - want).max()), float(np.abs(got1 - want[:1]).max()), float(np.abs(t32 - want).max())
    print(f"lstm: max |device - f64| = {err17:.3g} (P = 17), {err1:.3g} (P = 1); torch float32 LSTM vs f64 = {err_t:.3g}; bound 1e-4")
    assert np.abs(np.linalg.norm(got17, axis=1) - 1.0).max() <= 1e-6
    assert err17 <= 1e-4 and err1 <= 1e-4
    assert same_bits(got17[:1], got1)                                          # a partial's bits do not depend on its neighbours
    # ... nor on its row in the tile: partial 0 moved to the ragged second tile of a 17-partial call
    moved = emb.debug_lstm(np.concatenate([parts[1:], parts[:1]]))
    assert same_bits(moved[16:], got1) and same_bits(moved[:16], got17[1:])


# ------------------------------------------------------------------------------------------------ 3. end to end
def test_end_to_end_batch(emb):
    clips, want, want_parts = e2e_case()
    assert want_parts == [1, 2, 17]                                            # 20 partials: a tile of 16 spans clips, the second is ragged
    got, parts = emb.batch_partials(clips, 16000)
    err = float(np.abs(got - want).max())
    print(f"end to end: max |device - oracle| = {err:.3g}, bound 1e-4")
    assert parts.tolist() == want_parts and got.shape == (3, 256) and got.dtype == np.float32
    assert err <= 1e-4
    assert np.abs(np.linalg.norm(got.astype(np.float64), axis=1) - 1.0).max() <= 1e-6
    assert same_bits(emb.batch(clips, 16000), got)                             # the ``embed`` contract of make_forest_scorer
    for i, x in enumerate(clips):                                              # alone = in the batch = in a reordered batch
        assert same_bits(emb(x, 16000), got[i]) and same_bits(emb.batch([torch.from_numpy(x)], 16000)[0], got[i])
    order = [2, 0, 1]
    assert same_bits(emb.batch([clips[i] for i in order], 16000), got[order])


def test_a_24_khz_clip_goes_through_the_resampler(emb):
    rng = np.random.default_rng(23)
    n = 30000
    t = np.arange(n) / 24000.0
    x = (0.05 * np.sin(2 * np.pi * 180.0 * t) * (0.6 + 0.4 * np.sin(2 * np.pi * 2.7 * t)) + 0.01 * rng.standard_normal(n)).astype(np.float32)
    x16 = OW.resample(x, 24000, 16000)
    want, want_parts = R.embed(R.state(), x16)
    got, parts = emb.batch_partials([x], 24000)
    err = float(np.abs(got[0] - want).max())
    print(f"24 kHz: max |device - oracle| = {err:.3g}, bound 1e-4")
    assert parts.tolist() == [want_parts] and len(x16) == 20000 and err <= 1e-4
    mixed, _ = emb.batch_partials([x, x[:9001]], 24000)
    assert same_bits(mixed[0], got[0])


# ------------------------------------------------------------------------------------------------ 4. voice flags
def test_voice_flags_trim_long_silences(emb):
    n_win = 60
    x = voice(480 * n_win + 100, 31, 0.3)
    x[480 * 20: 480 * 40] *= 1e-3                                              # a silent middle
    flags = np.ones(n_win, dtype=np.int64)
    flags[20:40] = 0
    mask = S.smooth_voice_flags(flags)
    assert 0 < mask.sum() < n_win                                              # something is cut, something is kept
    want, want_parts = R.embed(R.state(), x, flags)
    got, parts = emb.batch_partials([x], 16000, voice_flags=[flags])
    plain, _ = emb.batch_partials([x], 16000)
    err = float(np.abs(got[0] - want).max())
    print(f"voice flags: max |device - oracle| = {err:.3g}, bound 1e-4; |with - without| = {float(np.abs(got[0] - plain[0]).max()):.3g}")
    assert parts.tolist() == [want_parts] and err <= 1e-4
    # the cut changes the embedding: by more than twice the oracle bound, so the two cannot both pass against one oracle value
    # (seeded weights spread embeddings little: unrelated clips lie within a few 1e-2 of each other)
    assert np.abs(got[0] - plain[0]).max() > 2e-4
    _, n_pre = emb.debug_mel(x, 16000, flags)
    assert n_pre == 480 * int(mask.sum())
    # all voiced: only the cut to a multiple of 480 (the clip is above -30 dBFS, so neither side is scaled)
    ones, _ = emb.batch_partials([x], 16000, voice_flags=[np.ones(n_win)])
    cut, _ = R.embed(R.state(), x[: 480 * n_win])
    assert np.abs(ones[0] - cut).max() <= 1e-4
    # nothing voiced: one partial of zeros, a finite embedding
    none, parts0 = emb.batch_partials([x], 16000, voice_flags=[np.zeros(n_win)])
    want0, _ = R.embed(R.state(), x, np.zeros(n_win))
    assert parts0.tolist() == [1] and np.isfinite(none).all() and np.abs(none[0] - want0).max() <= 1e-4
    # the vad hook supplies the flags of clips that come without
    hooked = S.SpeakerEmbedder(emb.ctx, synthetic=True, vad=lambda audio, sr: flags)
    try:
        assert same_bits(hooked.batch([x], 16000), got)
    finally:
        hooked.close()


def test_host_side_integer_decisions_equal_the_python_definitions(emb):
    """The native call decides partial counts and the trim mask on the host, in C++: held to ``partial_slices`` at the lengths where
    the last partial is kept, dropped or alone, and to ``smooth_voice_flags`` on random flags."""
    rng = np.random.default_rng(9)
    lengths = [8000, 37000, 38000, 208000, 217600, 224000, 1, 159, 160, 25599, 25600, 25601, 37919, 37920]
    clips = [(0.05 * rng.standard_normal(n)).astype(np.float32) for n in lengths]
    _, parts = emb.batch_partials(clips, 16000)
    assert parts.tolist() == [len(S.partial_slices(n)[0]) for n in lengths]
    x = (0.05 * rng.standard_normal(480 * 40 + 7)).astype(np.float32)
    for p in (0.2, 0.5, 0.8):
        flags = (rng.random(40) < p).astype(np.uint8)
        _, n_pre = emb.debug_mel(x, 16000, flags)
        assert n_pre == 480 * int(S.smooth_voice_flags(flags).sum()), (p, flags.tolist())


def test_refusals_before_any_launch(emb):
    x = voice(4800, 5)
    with pytest.raises(ValueError, match="voice flags"):
        emb.batch([x], 16000, voice_flags=[np.ones(9)])                        # 10 windows
    with pytest.raises(ValueError):
        emb.batch([x, np.zeros(0, dtype=np.float32)], 16000)                   # an empty clip
    assert np.isfinite(emb.batch([np.zeros(100, dtype=np.float32), x[:1]], 16000)).all()      # silence and one sample: no NaN


# ------------------------------------------------------------------------------------------------ 5. the 286-d vector
def _provider(**kw):
    from rho_tts_amd.provider import MI355XQwenTTS
    return MI355XQwenTTS(device="cuda", batch_size=4, max_iterations=2, **kw)


def test_the_provider_assembles_embedding_then_features(ctx, emb, tmp_path):
    enc = str(tmp_path / "encoder.npz")
    S.save(enc, R.state())
    audios = [torch.from_numpy(voice(30000 + 5000 * i, 40 + i)) for i in range(4)]
    ex = PF.HandcraftedFeatures(ctx)
    try:
        feats = ex.batch(audios, 24000)
    finally:
        ex.close()
    e = emb.batch(audios, 24000).astype(np.float64)
    x = np.concatenate([e, feats], axis=1)                                     # trainer.py:61-65: the embedding first
    assert x.shape == (4, 286)
    med = np.median(x, axis=0)
    leaf = FC.LEAF
    # splits on both sides of the seam, at the median of the four clips' values, so that every tree separates them
    trees = [[(f, float(med[f]), 2), (leaf, 0.1 + 0.05 * k, -1), (leaf, 0.9 - 0.07 * k, -1)] for k, f in enumerate((3, 255, 256, 269, 282, 285, 100, 257))]
    tables = F.validate(FC.tables_of(286, [trees]))
    path = str(tmp_path / "drift286.npz")
    F.save(path, tables)
    want = F.predict_host(tables, x)
    swapped = F.predict_host(tables, np.concatenate([feats, e], axis=1))
    assert not np.array_equal(want, swapped)                                   # (the check can tell the order)
    t = _provider(speaker="Vivian", model_path="x/CustomVoice-small", drift_model_path=path, speaker_encoder_path=enc)
    try:
        scorer = t.drift_scorer
        assert scorer is t.drift_scorer and t.drift_embed is None and t._speaker_embedder is not None
        got = scorer.batch(audios, 24000)
        assert got == [float(v) for v in want]
        assert scorer(audios[1], 24000) == float(want[1])
    finally:
        t.close()
    assert t._speaker_embedder is None and t._drift_native is None             # close() released what it made
    t = _provider(speaker="Vivian", model_path="x/CustomVoice-small", drift_model_path=path)
    try:
        with pytest.raises(ValueError, match="which this provider does not compute - set drift_embed"):
            t.drift_scorer
    finally:
        t.close()


# ------------------------------------------------------------------------------------------------ 6. speaker similarity
def test_ge2e_speaker_similarity(emb, tmp_path):
    enc, ref_path = str(tmp_path / "encoder.npz"), str(tmp_path / "ref.wav")
    S.save(enc, R.state())
    pcm = np.round(voice(40000, 51, 0.4) * 32767.0).astype("<i2")
    with wave.open(ref_path, "wb") as wf:
        wf.setnchannels(1)
        wf.setsampwidth(2)
        wf.setframerate(24000)
        wf.writeframes(pcm.tobytes())
    ref = pcm.astype(np.float32) / 32768.0
    t = _provider(reference_audio=ref_path, reference_text="a reference", model_path="x/Base-small", speaker_encoder_path=enc, speaker_similarity="ge2e")
    try:
        assert t.sample_rate == 24000                                          # (no engine is loaded: the file and the outputs are 24-kHz audio)
        other = voice(36000, 52, 0.2)
        sim = t._compute_speaker_similarity(torch.from_numpy(other))
        want_ref, _ = R.embed(R.state(), OW.resample(ref, 24000, 16000))
        want_other, _ = R.embed(R.state(), OW.resample(other, 24000, 16000))
        print(f"ge2e similarity: device {sim:.6f}, oracle {float(want_ref @ want_other):.6f}")
        assert abs(sim - float(want_ref @ want_other)) <= 1e-4
        assert t._ge2e_ref is not None and np.abs(t._ge2e_ref[1] - want_ref).max() <= 1e-4     # cached per voice
        cached = t._ge2e_ref[1]
        t._compute_speaker_similarity(torch.from_numpy(other))
        assert t._ge2e_ref[1] is cached
        assert abs(t._compute_speaker_similarity(torch.from_numpy(ref)) - 1.0) <= 1e-6         # the reference clip against itself
    finally:
        t.close()
    assert t._speaker_embedder is None
