"""Speed and pitch control on the GPU (``generate(..., speed=, pitch_semitones=)``, base_tts.py:618-650).

The reference hands both to torchaudio: ``functional.resample(audio, int(sr * speed), sr)`` and then
``functional.pitch_shift(audio, sr, steps)`` (STFT 512 / hop 128 -> phase vocoder -> inverse STFT -> resample back).  Here the same
two algorithms run in csrc/speedpitch.hip behind ``rt_speedpitch_apply``, evaluated in float64 between the float32 PCM that comes in
and the float32 PCM that goes out: the resampler's taps come from their closed form per output sample (torchaudio materialises a
[new][orig + 2 width] filter bank - 726 MB for +4 semitones at 24 kHz), and the vocoder's phase is accumulated in float64
(torchaudio: float32).  The definition is torchaudio 2.x's algorithm in exact arithmetic, restated in tests/speed_pitch_ref.py;
parity with the package itself is UNPINNED (not installable here).

Every integer decision - the reduced rates, the filter half-width, every length, ``int()``, ``round()``, ``ceil()`` - is taken HERE,
in ``plan``, with torchaudio's own Python expressions; the device gets integers and one double and decides nothing, so a call
needs no device-to-host copy.  ``plan`` is importable and usable without a GPU.
"""
from __future__ import annotations

import ctypes as C
import math

import torch

from . import _native

N_FFT, HOP, LOWPASS_WIDTH, ROLLOFF = 512, 128, 6, 0.99


class Plan(C.Structure):
    """rt_speedpitch_plan (include/rho_tts_amd.h)."""
    _fields_ = [("do_speed", C.c_int32), ("do_pitch", C.c_int32),
                ("s_o", C.c_int64), ("s_n", C.c_int64), ("s_width", C.c_int64), ("s_len", C.c_int64),
                ("L", C.c_int64), ("nf", C.c_int64), ("n_out", C.c_int64), ("ls", C.c_int64),
                ("p_o", C.c_int64), ("p_n", C.c_int64), ("p_width", C.c_int64), ("p_len", C.c_int64),
                ("rate", C.c_double)]

    @property
    def n_result(self) -> int:
        """Samples the call writes."""
        return int(self.L)


def _resample_terms(orig: int, new: int):
    """(o, n, width) of functional.resample(., orig, new); (1, 1, 0) for equal rates, where it returns its input."""
    if orig <= 0 or new <= 0:
        raise ValueError(f"Original frequency and desired frequecy should be positive (got {orig} -> {new})")
    if orig == new:
        return 1, 1, 0
    g = math.gcd(orig, new)
    o, n = orig // g, new // g
    base = min(o, n) * ROLLOFF
    return o, n, int(math.ceil(LOWPASS_WIDTH * o / base))


def plan(n: int, sample_rate: int, speed: float, pitch_semitones: float) -> Plan:
    """The host half of ``_apply_speed_pitch`` for a clip of ``n`` samples: which stages run and every integer they need."""
    n, sr = int(n), int(sample_rate)
    if n < 1:
        raise ValueError("speed / pitch: empty clip")
    p = Plan()
    L = n
    if speed != 1.0:
        orig = int(sr * speed)
        p.do_speed = 1
        p.s_o, p.s_n, p.s_width = _resample_terms(orig, sr)
        L = n if p.s_o == p.s_n else -(-p.s_n * n // p.s_o)
        p.s_len = L
    p.L = L
    if pitch_semitones != 0.0:
        if L <= N_FFT // 2:
            raise RuntimeError(f"pitch shift: reflect padding by {N_FFT // 2} needs a clip of more than {N_FFT // 2} samples, got {L}")
        rate = 2.0 ** (-float(pitch_semitones) / 12)
        p.do_pitch = 1
        p.rate = rate
        p.nf = 1 + L // HOP
        p.n_out = int(math.ceil(p.nf / rate))
        p.ls = int(round(L / rate))
        orig = int(sr / rate)
        p.p_o, p.p_n, p.p_width = _resample_terms(orig, sr)
        p.p_len = p.ls if p.p_o == p.p_n else -(-p.p_n * p.ls // p.p_o)
    return p


_DECLARED = False


def _declare(lib: C.CDLL) -> None:
    global _DECLARED
    if _DECLARED:
        return
    vp, i64 = C.c_void_p, C.c_int64
    lib.rt_speedpitch_create.argtypes = [vp, C.POINTER(vp)]
    lib.rt_speedpitch_destroy.argtypes = [vp]
    lib.rt_speedpitch_apply.argtypes = [vp, vp, i64, C.POINTER(Plan), vp, i64]
    _DECLARED = True


class SpeedPitch:
    """One ``rt_speedpitch`` (tables + grow-only workspaces) on a context."""

    def __init__(self, ctx: "_native.Context"):
        self.ctx, self.lib = ctx, ctx.lib
        _declare(self.lib)
        h = C.c_void_p()
        ctx.check(self.lib.rt_speedpitch_create(ctx.handle, C.byref(h)), "rt_speedpitch_create")
        self.handle = h

    def close(self) -> None:
        if getattr(self, "handle", None):
            self.lib.rt_speedpitch_destroy(self.handle)
            self.handle = None

    def _row(self, x: torch.Tensor, sample_rate: int, speed: float, steps: float) -> torch.Tensor:
        p = plan(x.numel(), sample_rate, speed, steps)
        out = torch.empty(p.n_result, dtype=torch.float32, device=x.device)
        self.ctx.check(self.lib.rt_speedpitch_apply(self.handle, C.c_void_p(x.data_ptr()), x.numel(), C.byref(p), C.c_void_p(out.data_ptr()),
                                                    out.numel()), "rt_speedpitch_apply")
        return out

    def __call__(self, audio: torch.Tensor, speed: float, pitch_semitones: float, sample_rate: int = 24000) -> torch.Tensor:
        """``BaseTTS._apply_speed_pitch`` (base_tts.py:618-650): a 1-D clip stays 1-D, [1][n] gives [1][n'], several rows are
        processed row by row.  (One difference in shape only: the reference squeezes a [1][n] clip to 1-D behind its speed stage,
        :637-638, and returns it 2-D from the pitch stage alone; here the rank of the input is kept in both.)  A device tensor stays
        on the device, a CPU tensor is moved over and its result moved back."""
        if speed == 1.0 and pitch_semitones == 0.0:
            return audio
        if audio.dim() not in (1, 2):
            raise ValueError(f"speed / pitch: expected a 1-D or 2-D waveform, got {tuple(audio.shape)}")
        dev = torch.device(f"cuda:{self.ctx.device_ordinal}")
        rows = audio.detach().to(device=dev, dtype=torch.float32).reshape(-1, audio.shape[-1]).contiguous()
        torch.cuda.current_stream(dev).synchronize()           # the context's stream is not torch's: the input is complete ...
        outs = [self._row(r, int(sample_rate), float(speed), float(pitch_semitones)) for r in rows]
        self.ctx.synchronize()                                 # ... and so is the output before torch reads it
        out = outs[0] if audio.dim() == 1 else torch.stack(outs)
        return out if audio.is_cuda else out.cpu()
