"""Speed / pitch control on the GPU (csrc/speedpitch.hip through rho_tts_amd/speedpitch.py and the provider) against the float64
restatement of torchaudio's algorithm (tests/speed_pitch_ref.py).

The bar of every comparison: lengths exact, max|gpu - ref64| <= 2 * 2^-23 * max(1, max|ref64|).  The kernels work in float64 and
round once, when they store the float32 result (half an ulp); the rest is float64 noise far below that.  torchaudio itself
evaluates in float32 and accumulates the vocoder's phase there: the yardstick test prints how far that is from the exact result.
"""
import functools
import wave

import numpy as np
import pytest
import torch

from rho_tts_amd import _native, api, speedpitch
from rho_tts_amd.provider import MI355XQwenTTS, register
from tests import speed_pitch_ref as R

pytestmark = pytest.mark.gpu
SR = 24000
BAR = 2.0 * 2.0 ** -23


def clip(L, seed=0):
    t = np.arange(L) / SR
    g = np.random.default_rng(1000 + 7 * L + seed)
    x = (0.4 * np.sin(2 * np.pi * 180.0 * t) * (0.6 + 0.4 * np.sin(2 * np.pi * 3.0 * t)) + 0.15 * np.sin(2 * np.pi * 1310.0 * t + 0.3) +
         0.05 * g.standard_normal(L))
    return x.astype(np.float32)


@functools.lru_cache(maxsize=None)
def case(L, speed, steps):
    """(float32 clip, its float64 result): computed once, shared by the tests, never written to."""
    x = clip(L)
    ref = R.apply_speed_pitch(x.astype(np.float64), SR, speed, steps)
    x.setflags(write=False)
    ref.setflags(write=False)
    return x, ref


@pytest.fixture(scope="module")
def sp():
    ctx = _native.Context(0)
    s = speedpitch.SpeedPitch(ctx)
    yield s
    s.close()
    ctx.close()


def run(sp, x, speed, steps):
    return sp(torch.from_numpy(np.array(x)).cuda(), speed, steps, sample_rate=SR).cpu().numpy()


def within_bar(got, ref, what):
    assert got.dtype == np.float32 and got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.isfinite(got).all(), what
    err = float(np.abs(got.astype(np.float64) - ref).max()) if ref.size else 0.0
    bound = BAR * max(1.0, float(np.abs(ref).max()) if ref.size else 0.0)
    print(f"{what}: max|gpu - ref64| = {err:.3g} (bar {bound:.3g})")
    assert err <= bound, (what, err, bound)


@pytest.mark.parametrize("speed", [2, 0.5, 1.1, 0.9, 1.07, 3.3])
def test_resample_alone(sp, speed):
    for L in (1, 5, 300, 4001):
        x, ref = case(L, float(speed), 0.0)
        within_bar(run(sp, x, float(speed), 0.0), ref, f"speed {speed} L {L}")


def test_equal_rates_return_the_input_bit_for_bit(sp):
    for L in (1, 300, 4001):
        x = clip(L)
        got = run(sp, x, 1.00001, 0.0)                         # int(24000 * 1.00001) == 24000
        assert got.tobytes() == x.tobytes()


@pytest.mark.parametrize("steps", [4, -3, 12, -12, 0.5, 7.3])
def test_pitch_alone(sp, steps):
    # (24000 samples an octave up are 376 output frames: several per lane of the vocoder's wave scan; 257 is the shortest legal clip;
    # 0.5 and 7.3 semitones are ratios whose reduced terms are in the tens of thousands)
    assert speedpitch.plan(24000, SR, 1.0, 12.0).n_out == 376 and speedpitch.plan(24000, SR, 1.0, 0.5).p_o == 24703
    for L in (257, 300, 600, 4001, 24000):
        x, ref = case(L, 1.0, float(steps))
        within_bar(run(sp, x, 1.0, float(steps)), ref, f"steps {steps} L {L}")


def test_special_signals(sp):
    L = 1500
    zeros = np.zeros(L, dtype=np.float32)
    first, last, const = zeros.copy(), zeros.copy(), np.full(L, 0.25, dtype=np.float32)
    first[0], last[-1] = 1.0, 1.0
    padded = clip(L).copy()
    padded[:400], padded[-350:] = 0.0, 0.0
    for speed, steps in ((1.1, 0.0), (1.0, 4.0), (1.0, -3.0), (0.9, 7.3)):
        got = run(sp, zeros, speed, steps)
        assert np.isfinite(got).all() and not got.any(), (speed, steps)
        for name, x in (("impulse at 0", first), ("impulse at the end", last), ("constant", const), ("zeros around", padded)):
            within_bar(run(sp, x, speed, steps), R.apply_speed_pitch(x.astype(np.float64), SR, speed, steps), f"{name}, speed {speed} steps {steps}")


def test_closer_to_the_exact_result_than_torchaudios_float32_evaluation(sp):
    """rms(gpu - ref64) < rms(ref32 - ref64) at +4 semitones, ref32 = the dense float32 form torchaudio runs (its phase accumulator
    drifts with the clip's length: about 1.7e-6 / 1.3e-5 / 4.1e-5 at these lengths)."""
    Ls = (600, 4000, 24000)
    ref32 = R.pitch_shift_dense([torch.from_numpy(np.array(case(L, 1.0, 4.0)[0])) for L in Ls], SR, 4.0, torch.float32)
    for L, r32 in zip(Ls, ref32):
        x, ref = case(L, 1.0, 4.0)
        got = run(sp, x, 1.0, 4.0)
        e_gpu = float(np.sqrt(np.mean((got.astype(np.float64) - ref) ** 2)))
        e_f32 = float(np.sqrt(np.mean((r32.numpy().astype(np.float64) - ref) ** 2)))
        print(f"+4 semitones L {L}: rms(gpu - ref64) = {e_gpu:.3g}, rms(float32 dense - ref64) = {e_f32:.3g}")
        assert e_gpu < e_f32, (L, e_gpu, e_f32)


def test_native_call_refuses_an_inconsistent_plan_or_a_short_buffer(sp):
    import ctypes as C
    x = torch.from_numpy(clip(1000)).cuda()
    out = torch.full((2000,), 7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()

    def call(p, cap):
        return sp.lib.rt_speedpitch_apply(sp.handle, C.c_void_p(x.data_ptr()), x.numel(), C.byref(p), C.c_void_p(out.data_ptr()), cap)

    good = speedpitch.plan(1000, SR, 1.1, 4.0)
    assert call(good, good.n_result - 1) == _native.RT_ERR_INVALID
    for field, value in (("s_len", good.s_len + 1), ("s_width", good.s_width - 1), ("s_o", good.s_o * 2), ("L", good.L - 1), ("nf", good.nf + 1),
                         ("n_out", good.n_out + 3), ("ls", good.ls + 5), ("p_len", good.p_len - 1), ("p_o", good.p_o * 3), ("rate", 0.0)):
        bad = speedpitch.plan(1000, SR, 1.1, 4.0)
        setattr(bad, field, value)
        assert call(bad, 2000) == _native.RT_ERR_INVALID, field
    short = speedpitch.plan(300, SR, 1.0, 4.0)                 # a pitch stage on 200 samples: the plan of a longer clip does not pass
    assert sp.lib.rt_speedpitch_apply(sp.handle, C.c_void_p(x.data_ptr()), 200, C.byref(short), C.c_void_p(out.data_ptr()), 2000) == _native.RT_ERR_INVALID
    sp.ctx.synchronize()
    assert bool((out == 7.0).all())                            # nothing was written by any refused call
    assert call(good, 2000) == _native.RT_OK
    sp.ctx.synchronize()
    assert bool((out[good.n_result:] == 7.0).all()) and not bool((out[: good.n_result] == 7.0).any())


def test_through_the_provider():
    p = MI355XQwenTTS(model_path="tiny")
    try:
        x, ref = case(4001, 1.1, -3.0)                          # speed first, then pitch
        xt = torch.from_numpy(np.array(x))
        a = p._apply_speed_pitch(xt.cuda(), 1.1, -3.0)
        assert a.is_cuda and a.dim() == 1
        within_bar(a.cpu().numpy(), ref, "provider, 1-D on the device")
        b = p._apply_speed_pitch(xt.cuda().unsqueeze(0), 1.1, -3.0)
        assert b.is_cuda and b.shape == (1, ref.shape[0]) and torch.equal(b[0], a)
        c = p._apply_speed_pitch(xt, 1.1, -3.0)
        assert not c.is_cuda and torch.equal(c, a.cpu())
        two = p._apply_speed_pitch(torch.stack([xt, -xt]), 1.0, 4.0)
        assert two.shape == (2, 4001)
        within_bar(two[0].numpy(), case(4001, 1.0, 4.0)[1], "provider, row 0 of two")
        within_bar(two[1].numpy(), R.apply_speed_pitch(-x.astype(np.float64), SR, 1.0, 4.0), "provider, row 1 of two")
        assert p._apply_speed_pitch(xt, 1.0, 0.0) is xt
        with pytest.raises(RuntimeError):
            p._apply_speed_pitch(xt[:200], 1.0, 2.0)
        with pytest.raises(ValueError):
            p._apply_speed_pitch(xt, 0.0, 0.0)
        # loading the engine replaces the context the first calls ran on: the state object goes with it and the next call makes its own
        first = p._speed_pitch
        assert first is not None and p._engine is None
        p._load_engine()
        assert p._speed_pitch is None and first.handle is None
        assert torch.equal(p._apply_speed_pitch(xt, 1.1, -3.0), c) and p._speed_pitch.ctx is p._engine.ctx
    finally:
        p.close()
    assert p._speed_pitch is None


@pytest.fixture(scope="module")
def small_provider(tmp_path_factory):
    d = tmp_path_factory.mktemp("voice")
    ref = d / "ref.wav"
    i = np.arange(SR * 2)
    pcm = (0.3 * np.sin(2 * np.pi * 150 * i / SR) * (0.6 + 0.4 * np.sin(2 * np.pi * 3 * i / SR)) * 32767).astype("<i2")
    with wave.open(str(ref), "wb") as wf:
        wf.setnchannels(1); wf.setsampwidth(2); wf.setframerate(SR); wf.writeframes(pcm.tobytes())
    saved = dict(api.TTSFactory._providers)
    name = register()
    p = api.TTSFactory.get_tts_instance(name, reference_audio=str(ref), reference_text="a short reference sentence", model_path="small", batch_size=4)
    yield p
    p.close()
    api.TTSFactory._providers = saved


def test_generate_with_speed_and_pitch_end_to_end(small_provider):
    p = small_provider
    text = "Hello there general test of the path"
    plain = p.generate(text)
    assert plain is not None and plain.audio.dim() == 1
    shifted = p.generate(text, speed=1.25, pitch_semitones=-2)
    again = p.generate(text)
    assert torch.equal(plain.audio.cpu(), again.audio.cpu())    # the defaults never reach the new code: bit-identical before and after
    ref = R.apply_speed_pitch(plain.audio.cpu().numpy().astype(np.float64), p.sample_rate, 1.25, -2)
    assert ref.shape[0] == -(-plain.audio.numel() * 4 // 5)     # 30000 : 24000 = 5 : 4
    within_bar(shifted.audio.cpu().numpy().reshape(-1), ref, "generate(speed=1.25, pitch_semitones=-2)")
    assert shifted.audio.device == plain.audio.device
    assert abs(shifted.duration_sec - ref.shape[0] / p.sample_rate) < 1e-9
    parts = list(p.stream(text, speed=1.25, pitch_semitones=-2))
    assert len(parts) == 1 and parts[0].audio.numel() > 0
    assert abs(parts[0].duration_sec - parts[0].audio.numel() / p.sample_rate) < 1e-9
