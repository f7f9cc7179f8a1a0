"""The definition the speed / pitch tests compare against (tests/test_speed_pitch_cpu.py, tests/test_speed_pitch_gpu.py).

torchaudio 2.x's ``functional.resample`` (sinc_interp_hann, lowpass_filter_width 6, rolloff 0.99) and ``functional.pitch_shift``
(n_fft 512, hop 128, periodic Hann, 12 bins per octave), restated twice:

* ``resample`` / ``pitch_shift`` / ``apply_speed_pitch``: numpy float64, the resampler's taps evaluated per output sample from
  their closed form.  This is what the HIP kernels are held to (the reference called ``ref64`` in the tests).
* ``resample_dense`` / ``pitch_shift_dense`` / ``apply_dense``: the dense form torchaudio itself runs - a [new][orig + 2 width]
  filter bank applied with ``conv1d``, ``torch.stft`` / ``torch.istft`` around the phase vocoder - in a dtype of the caller's
  choice: float64 as a cross-check of the form above, float32 as "torchaudio as its users run it".  The filter bank is built and
  applied a block of phases at a time, so that a ratio whose reduced terms are in the tens of thousands does not need gigabytes.

torchaudio is not installed where these tests run: parity with the package itself is UNPINNED; both forms restate its source.
"""
from __future__ import annotations

import math
from typing import List, Sequence

import numpy as np
import torch

N_FFT, HOP, WIDTH, ROLLOFF = 512, 128, 6, 0.99
N_BINS = N_FFT // 2 + 1


# ------------------------------------------------------------------------------------------------ integer decisions
def resample_geometry(orig: int, new: int):
    """(o, n, width, base, scale) of a rate pair; o == n == 1 for equal rates (the resampler returns its input)."""
    orig, new = int(orig), int(new)
    if orig <= 0 or new <= 0:
        raise ValueError("Original frequency and desired frequecy should be positive")
    g = math.gcd(orig, new)
    o, n = orig // g, new // g
    base = min(o, n) * ROLLOFF
    return o, n, int(math.ceil(WIDTH * o / base)), base, base / o


def resample_length(L: int, orig: int, new: int) -> int:
    o, n = resample_geometry(orig, new)[:2]
    return int(L) if o == n else -(-n * int(L) // o)


def pitch_geometry(L: int, sr: int, steps: float):
    """(rate, nf, n_out, ls, orig) of the pitch stage of an L-sample clip."""
    if L <= N_FFT // 2:
        raise RuntimeError(f"pitch shift: reflect padding by {N_FFT // 2} needs more than {N_FFT // 2} samples, got {L}")
    rate = 2.0 ** (-float(steps) / 12)
    nf = 1 + L // HOP
    return rate, nf, int(math.ceil(nf / rate)), int(round(L / rate)), int(sr / rate)


def lengths(n: int, sr: int, speed: float, steps: float) -> dict:
    """Every length the two stages decide, as ``rho_tts_amd.speedpitch.plan`` must reproduce them."""
    out = {"n_in": int(n), "speed": speed != 1.0, "pitch": steps != 0.0}
    L = int(n)
    if speed != 1.0:
        o, nn, w = resample_geometry(int(sr * speed), sr)[:3]
        L = resample_length(L, int(sr * speed), sr)
        out.update(s_o=o, s_n=nn, s_width=w, s_len=L)
    if steps != 0.0:
        rate, nf, n_out, ls, orig = pitch_geometry(L, sr, steps)
        o, nn, w = resample_geometry(orig, sr)[:3]
        out.update(L=L, rate=rate, nf=nf, n_out=n_out, ls=ls, p_o=o, p_n=nn, p_width=w, p_len=resample_length(ls, orig, sr))
    out["n_result"] = L
    return out


# ------------------------------------------------------------------------------------------------ float64, taps on the fly
def resample(x: np.ndarray, orig: int, new: int) -> np.ndarray:
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    o, n, width, base, scale = resample_geometry(orig, new)
    if o == n:
        return x.copy()
    L = x.shape[0]
    n_out = -(-n * L // o)
    i = np.arange(n_out, dtype=np.int64)
    p, j = i % n, i // n
    c = (o * p) // n                                           # floor(o p / n): the tap whose t is nearest to zero from below
    y = np.zeros(n_out)
    for k in range(-width, width + 2):                         # ascending k; |t| >= 6 outside this run
        kk = c + k                                             # = k - width of the definition
        t = (-(p.astype(np.float64)) / n + kk.astype(np.float64) / o) * base
        live = (np.abs(t) < WIDTH) & (kk + width < 2 * width + o)
        t = np.clip(t, -WIDTH, WIDTH)
        with np.errstate(divide="ignore", invalid="ignore"):
            s = np.where(t == 0.0, 1.0, np.sin(np.pi * t) / (np.pi * t))
        h = s * np.cos(np.pi * t / (2 * WIDTH)) ** 2 * scale
        src = j * o + kk
        ok = live & (src >= 0) & (src < L)
        y += np.where(ok, h * x[np.clip(src, 0, L - 1)], 0.0)
    return y


def hann() -> np.ndarray:
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(N_FFT) / N_FFT)


def stft(x: np.ndarray) -> np.ndarray:
    """[257][nf] complex128: centred, reflect-padded frames times the periodic Hann window."""
    L = x.shape[0]
    nf = 1 + L // HOP
    xp = np.pad(x, N_FFT // 2, mode="reflect")
    fr = np.lib.stride_tricks.as_strided(xp, shape=(nf, N_FFT), strides=(HOP * xp.strides[0], xp.strides[0]))
    return np.fft.rfft(fr * hann()[None, :], axis=1).T


def phase_vocoder(S: np.ndarray, rate: float) -> np.ndarray:
    nf = S.shape[1]
    n_out = int(math.ceil(nf / rate))
    ts = np.arange(n_out, dtype=np.float64) * rate
    f0 = np.floor(ts).astype(np.int64)
    alpha = ts - f0
    Sp = np.concatenate([S, np.zeros((S.shape[0], 2), dtype=S.dtype)], axis=1)
    s0, s1 = Sp[:, f0], Sp[:, f0 + 1]
    pa = (np.arange(N_BINS, dtype=np.float64) * (np.pi * HOP / (N_BINS - 1)))[:, None]
    mag = alpha[None, :] * np.abs(s1) + (1.0 - alpha[None, :]) * np.abs(s0)
    d = np.angle(s1) - np.angle(s0) - pa
    d = d - 2.0 * np.pi * np.round(d / (2.0 * np.pi)) + pa
    phase = np.cumsum(np.concatenate([np.angle(S[:, :1]), d[:, :-1]], axis=1), axis=1)
    return mag * (np.cos(phase) + 1j * np.sin(phase))


def istft(Z: np.ndarray, length: int) -> np.ndarray:
    n_out = Z.shape[1]
    w = hann()
    fr = np.fft.irfft(Z.T, n=N_FFT, axis=1) * w[None, :]
    total = N_FFT + HOP * (n_out - 1)
    y, env = np.zeros(total), np.zeros(total)
    for f in range(n_out):                                     # ascending frame order
        y[f * HOP: f * HOP + N_FFT] += fr[f]
        env[f * HOP: f * HOP + N_FFT] += w * w
    lo, hi = N_FFT // 2, min(N_FFT // 2 + length, total)
    out = np.zeros(length)
    if hi > lo:
        out[: hi - lo] = y[lo:hi] / env[lo:hi]
    return out


def stretch(x: np.ndarray, steps: float) -> np.ndarray:
    rate, _, _, ls, _ = pitch_geometry(x.shape[0], 1, steps)
    return istft(phase_vocoder(stft(x), rate), ls)


def pitch_shift(x: np.ndarray, sr: int, steps: float) -> np.ndarray:
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    L = x.shape[0]
    rate, _, _, _, orig = pitch_geometry(L, sr, steps)
    y = resample(stretch(x, steps), orig, sr)
    out = np.zeros(L)
    out[: min(L, y.shape[0])] = y[:L]
    return out


def apply_speed_pitch(x: np.ndarray, sr: int, speed: float, steps: float) -> np.ndarray:
    """``BaseTTS._apply_speed_pitch`` on one row, float64 throughout: speed first, then pitch."""
    y = np.asarray(x, dtype=np.float64).reshape(-1)
    if speed != 1.0:
        y = resample(y, int(sr * speed), sr)
    if steps != 0.0:
        y = pitch_shift(y, sr, steps)
    return y


# ------------------------------------------------------------------------------------------------ dense torch form
def resample_dense(xs: Sequence[torch.Tensor], orig: int, new: int, dtype=torch.float64, block: int = 512) -> List[torch.Tensor]:
    """torchaudio's evaluation for every signal of ``xs`` (1-D), the filter bank built ``block`` phases at a time."""
    xs = [x.to(dtype).reshape(-1) for x in xs]
    o, n, width, base, scale = resample_geometry(orig, new)
    if o == n:
        return [x.clone() for x in xs]
    idx = torch.arange(-width, width + o, dtype=dtype)[None, None] / o
    padded = [torch.nn.functional.pad(x, (width, width + o))[None, None] for x in xs]
    outs = [torch.zeros(x.numel() // o + 1, n, dtype=dtype) for x in xs]
    for p0 in range(0, n, block):
        p1 = min(n, p0 + block)
        t = torch.arange(-p0, -p1, -1, dtype=dtype)[:, None, None] / n + idx
        t *= base
        t = t.clamp_(-WIDTH, WIDTH)
        window = torch.cos(t * math.pi / WIDTH / 2) ** 2
        t *= math.pi
        kern = torch.where(t == 0, torch.tensor(1.0, dtype=dtype), t.sin() / t)
        kern *= window * scale
        for xp, out in zip(padded, outs):
            out[:, p0:p1] = torch.nn.functional.conv1d(xp, kern, stride=o)[0].T
    return [out.reshape(-1)[: -(-n * x.numel() // o)] for x, out in zip(xs, outs)]


def stretch_dense(x: torch.Tensor, steps: float, dtype=torch.float64) -> torch.Tensor:
    x = x.to(dtype).reshape(1, -1)
    L = x.shape[-1]
    rate = 2.0 ** (-float(steps) / 12)
    window = torch.hann_window(N_FFT, dtype=dtype)
    spec = torch.stft(x, n_fft=N_FFT, hop_length=HOP, win_length=N_FFT, window=window, center=True, pad_mode="reflect",
                      normalized=False, onesided=True, return_complex=True)
    pa = torch.linspace(0, math.pi * HOP, spec.shape[-2], dtype=dtype)[..., None]
    ts = torch.arange(0, spec.size(-1), rate, dtype=dtype)
    alphas = ts % 1.0
    phase_0 = spec[..., :1].angle()
    spec = torch.nn.functional.pad(spec, [0, 2])
    s0, s1 = spec.index_select(-1, ts.long()), spec.index_select(-1, (ts + 1).long())
    phase = s1.angle() - s0.angle() - pa
    phase = phase - 2 * math.pi * torch.round(phase / (2 * math.pi))
    phase = phase + pa
    phase_acc = torch.cumsum(torch.cat([phase_0, phase[..., :-1]], dim=-1), -1)
    mag = alphas * s1.abs() + (1 - alphas) * s0.abs()
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                        # (istft warns when `length` pads behind the last frame)
        return torch.istft(torch.polar(mag, phase_acc), n_fft=N_FFT, hop_length=HOP, win_length=N_FFT, window=window,
                           length=int(round(L / rate)))[0]


def pitch_shift_dense(xs: Sequence[torch.Tensor], sr: int, steps: float, dtype=torch.float64) -> List[torch.Tensor]:
    rate = 2.0 ** (-float(steps) / 12)
    ys = resample_dense([stretch_dense(x, steps, dtype) for x in xs], int(sr / rate), sr, dtype)
    outs = []
    for x, y in zip(xs, ys):
        L = x.numel()
        out = torch.zeros(L, dtype=dtype)
        out[: min(L, y.numel())] = y[:L]
        outs.append(out)
    return outs


def apply_dense(xs: Sequence[torch.Tensor], sr: int, speed: float, steps: float, dtype=torch.float64) -> List[torch.Tensor]:
    ys = [x.to(dtype).reshape(-1) for x in xs]
    if speed != 1.0:
        ys = resample_dense(ys, int(sr * speed), sr, dtype)
    if steps != 0.0:
        ys = pitch_shift_dense(ys, sr, steps, dtype)
    return ys
