"""Speed / pitch control, the host side (no GPU): the float64 restatement the kernels are held to agrees with the dense form
torchaudio runs, has the properties the reference's own tests/test_speed_pitch.py checks, and ``rho_tts_amd.speedpitch.plan``
takes every integer decision exactly as the restatement does."""
import numpy as np
import pytest
import torch

from rho_tts_amd import speedpitch
from tests import speed_pitch_ref as R

SR = 24000
LENGTHS = (5, 300, 600, 4000)


def clip(L, seed=0):
    """A voiced-looking clip: two partials under a slow envelope, plus noise."""
    t = np.arange(L) / SR
    g = np.random.default_rng(1000 + 7 * L + seed)
    return (0.4 * np.sin(2 * np.pi * 180.0 * t) * (0.6 + 0.4 * np.sin(2 * np.pi * 3.0 * t)) + 0.15 * np.sin(2 * np.pi * 1310.0 * t + 0.3) +
            0.05 * g.standard_normal(L))


@pytest.mark.parametrize("speed", [0.5, 0.9, 1.07, 1.1, 2])
def test_resample_taps_on_the_fly_equal_the_dense_form(speed):
    xs = [clip(L) for L in LENGTHS]
    dense = R.resample_dense([torch.from_numpy(x) for x in xs], int(SR * speed), SR, torch.float64)
    for x, d in zip(xs, dense):
        y = R.resample(x, int(SR * speed), SR)
        assert y.shape[0] == d.numel() == R.resample_length(x.shape[0], int(SR * speed), SR)
        err = float(np.abs(y - d.numpy()).max())
        print(f"speed {speed} L {x.shape[0]}: max|taps - dense| = {err:.3g}")
        assert err <= 1e-12


@pytest.mark.parametrize("steps", [12, -12, 4, -3])
def test_pitch_shift_taps_on_the_fly_equal_the_dense_form(steps):
    xs = [clip(L) for L in LENGTHS if L > 256]
    dense = R.pitch_shift_dense([torch.from_numpy(x) for x in xs], SR, steps, torch.float64)
    for x, d in zip(xs, dense):
        y = R.pitch_shift(x, SR, steps)
        assert y.shape[0] == d.numel() == x.shape[0]
        err = float(np.abs(y - d.numpy()).max())
        print(f"steps {steps} L {x.shape[0]}: max|taps - dense| = {err:.3g}")
        assert err <= 1e-12
    for L in (5, 256):                                         # both forms refuse what torch.stft's reflect padding refuses
        with pytest.raises(RuntimeError):
            R.pitch_shift(clip(L), SR, steps)
        with pytest.raises(RuntimeError):
            R.pitch_shift_dense([torch.from_numpy(clip(L))], SR, steps)


def test_the_references_own_properties():
    """tests/test_speed_pitch.py of the reference: a second of a 440-Hz sine at 16 kHz."""
    sr = 16000
    x = np.sin(2 * 3.14159 * 440 * np.linspace(0, 1, sr))
    fast, slow = R.apply_speed_pitch(x, sr, 2.0, 0.0), R.apply_speed_pitch(x, sr, 0.5, 0.0)
    assert 0.3 < fast.shape[0] / sr < 0.7 and fast.shape[0] == sr // 2
    assert 1.5 < slow.shape[0] / sr < 2.5 and slow.shape[0] == sr * 2
    assert R.apply_speed_pitch(x, sr, 1.0, 4.0).shape[0] == sr
    assert np.array_equal(R.apply_speed_pitch(x, sr, 1.0, 0.0), x)
    # ... and what the stages do to the tone: twice the speed doubles its frequency, +12 semitones too, at the same length
    def peak_hz(y):
        return float(np.argmax(np.abs(np.fft.rfft(y * np.hanning(y.shape[0])))) * sr / y.shape[0])
    assert abs(peak_hz(fast) - 880.0) < 4.0 and abs(peak_hz(slow) - 220.0) < 2.0
    assert abs(peak_hz(R.apply_speed_pitch(x, sr, 1.0, 12.0)) - 880.0) < 4.0


PLAN_LENGTHS = list(range(1, 5001, 131)) + [127, 128, 129, 255, 256, 257, 258, 383, 384, 385, 4999, 5000, 24000, 240000]
PLAN_FIELDS = ("s_o", "s_n", "s_width", "s_len", "L", "nf", "n_out", "ls", "p_o", "p_n", "p_width", "p_len")


def test_plan_equals_the_restatements_lengths():
    assert all(L % 128 for L in range(1, 5001, 131)[1:])
    for L in PLAN_LENGTHS:
        for speed in (1.0, 0.5, 0.9, 1.00001, 1.07, 1.1, 2, 3.3):
            for steps in (0.0, 12, -12, 4, -4, -3, 0.5, 7.3):
                if speed == 1.0 and steps == 0.0:
                    continue
                try:
                    want = R.lengths(L, SR, speed, steps)
                except RuntimeError:
                    with pytest.raises(RuntimeError):
                        speedpitch.plan(L, SR, speed, steps)
                    continue
                p = speedpitch.plan(L, SR, speed, steps)
                assert (bool(p.do_speed), bool(p.do_pitch)) == (want["speed"], want["pitch"])
                assert p.n_result == want["n_result"]
                for f in PLAN_FIELDS:
                    if f in want:
                        got = getattr(p, f)
                        if f.endswith(("_o", "_n", "_width")) and want[f[0] + "_o"] == want[f[0] + "_n"]:
                            continue                           # equal rates: the stage copies, the terms are not used
                        assert got == want[f], (L, speed, steps, f, got, want[f])
                if want["pitch"]:
                    assert p.rate == want["rate"]
    # the restatement's lengths are the lengths of what it returns
    for L, speed, steps in ((300, 1.07, 0.0), (600, 0.9, 4), (257, 1.0, -3), (4000, 3.3, 7.3), (1000, 1.00001, 0.0)):
        assert R.apply_speed_pitch(clip(L), SR, speed, steps).shape[0] == speedpitch.plan(L, SR, speed, steps).n_result


def test_plan_refuses_what_torchaudio_refuses():
    with pytest.raises(ValueError):
        speedpitch.plan(1000, SR, 0.0, 0.0)                    # int(sr * speed) == 0
    with pytest.raises(ValueError):
        speedpitch.plan(1000, SR, 0.00001, 2.0)
    with pytest.raises(ValueError):
        speedpitch.plan(1000, SR, -1.0, 0.0)
    with pytest.raises(RuntimeError):
        speedpitch.plan(256, SR, 1.0, 2.0)                     # reflect padding by 256 needs 257 samples
    with pytest.raises(RuntimeError):
        speedpitch.plan(600, SR, 3.3, 2.0)                     # ... of the clip the pitch stage sees: 182 after the speed stage
    assert speedpitch.plan(257, SR, 1.0, 2.0).nf == 3
    assert speedpitch.plan(200, SR, 2.0, 0.0).n_result == 100  # the speed stage alone takes any clip
    p = speedpitch.plan(1000, SR, 1.00001, 0.0)                # int(24000.24) == 24000: the resampler returns its input
    assert p.do_speed and p.s_o == p.s_n and p.n_result == 1000
