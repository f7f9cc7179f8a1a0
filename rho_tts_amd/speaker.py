"""The GE2E speaker encoder on the GPU: the 256-d embedding that completes the drift classifier's 286-d vector.

The reference's classifier scores ``[resemblyzer embedding (256) | 30 hand-crafted features]`` (validation/classifier/trainer.py:23-68)
and ``_compute_speaker_similarity`` (base_tts.py:325-346) is the dot product of two such embeddings.  ``features.py`` produces the 30;
this module produces the 256 from the waveform in HBM, in one native call per chunk of clips (``rt_spk_embed_batch``,
csrc/speaker.hip): resample to 16 kHz -> normalize_volume(-30 dBFS, increase only) -> optional trim_long_silences -> partial
utterances of 1.6 s every 77 frames -> 40-band power mel (n_fft 400, hop 160) -> 3 x LSTM-256 -> Linear-256 -> ReLU -> L2 norm ->
mean over the partials -> L2 norm.  1,423,616 parameters.

The definition is resemblyzer 0.1.x restated; parity with resemblyzer is UNPINNED - neither resemblyzer, webrtcvad nor librosa can
be installed here and no pretrained weights are available offline.  tests/speaker_embed_ref.py is the float64 oracle of what is
stated here.  Deviations, both deliberate:

* resemblyzer trims long silences with webrtcvad's voice flags (mode 3, 30-ms windows of int16).  No VAD is restated or replaced:
  the caller supplies one 0/1 flag per 480-sample window of the 16-kHz clip (``voice_flags=``, or a ``vad`` callable given to
  ``SpeakerEmbedder``), and everything behind the flags - moving average, rounding, dilation, compaction - is done here.  WITHOUT
  flags the stage is skipped and nothing is cut: that is the default.  A mask that keeps nothing yields one partial of zeros.
* a clip whose rms is 0 is left unchanged by the volume stage, where resemblyzer would divide by zero and produce NaN; a zero
  embedding norm likewise gives a zero vector.

Weights come from a ``.npz`` with torch's tensor names (tools/export_speaker_encoder.py writes it from resemblyzer's
``pretrained.pt``); the package never unpickles.  Without a file the encoder runs on seeded weights only when ``synthetic=True``.
"""
from __future__ import annotations

import ctypes as C
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _native

SR = 16000
DIM = 256
N_MELS, N_FFT, HOP = 40, 400, 160
HIDDEN, LAYERS = 256, 3
PARTIAL_FRAMES = 160                               # 1.6 s
RATE, MIN_COVERAGE = 1.3, 0.75
FRAME_STEP = int(np.round((SR / RATE) / HOP))      # 77
VAD_WINDOW = 480                                   # 30 ms at 16 kHz
VAD_AVERAGE, VAD_MAX_SILENCE = 8, 6
TARGET_DBFS = -30.0

_DECLARED = False


def _declare(lib: C.CDLL) -> None:
    global _DECLARED
    if _DECLARED:
        return
    vp, i32, i64, pf = C.c_void_p, C.c_int32, C.c_int64, C.POINTER(C.c_float)
    lib.rt_spk_create.argtypes = [vp, C.POINTER(vp)]
    lib.rt_spk_destroy.argtypes = [vp]
    lib.rt_spk_set_tensor.argtypes = [vp, C.c_char_p, pf, i64, i64]
    lib.rt_spk_finalize.argtypes = [vp]
    lib.rt_spk_embed_batch.argtypes = [vp, C.POINTER(vp), C.POINTER(i64), i32, i32, C.POINTER(vp), C.POINTER(i32), pf, C.POINTER(i32)]
    lib.rt_debug_spk_mel.argtypes = [vp, vp, i64, i32, vp, i32, pf, i32, C.POINTER(i32), C.POINTER(i64)]
    lib.rt_debug_spk_lstm.argtypes = [vp, pf, i32, pf]
    _DECLARED = True


# ------------------------------------------------------------------------------------------------ host definitions
def partial_slices(n_samples: int) -> Tuple[List[Tuple[int, int]], int]:
    """resemblyzer's ``compute_partial_slices(n, rate=1.3, min_coverage=0.75)``: the mel-frame ranges ``[start, stop)`` of the
    partial utterances of a 16-kHz clip of ``n_samples``, and the length the clip is zero-padded to (``n_samples`` itself when the
    last partial ends inside it)."""
    n = int(n_samples)
    n_frames = -(-(n + 1) // HOP)
    steps = max(1, n_frames - PARTIAL_FRAMES + FRAME_STEP + 1)
    slices = [(i, i + PARTIAL_FRAMES) for i in range(0, steps, FRAME_STEP)]
    if len(slices) > 1 and (n - HOP * slices[-1][0]) / (PARTIAL_FRAMES * HOP) < MIN_COVERAGE:
        slices = slices[:-1]
    return slices, max(n, HOP * slices[-1][1])


def smooth_voice_flags(flags) -> np.ndarray:
    """The mask of ``trim_long_silences`` behind the VAD: one 0/1 voice flag per 480-sample window -> one bool per window.  Moving
    average of width 8 (3 zeros in front, 4 behind, cumulative-sum difference), ``np.round`` (half to even: exactly 0.5 becomes 0),
    binary dilation with seven ones."""
    f = np.asarray(flags).astype(bool).astype(np.float64).reshape(-1)
    if f.size == 0:
        return np.zeros(0, dtype=bool)
    w = VAD_AVERAGE
    padded = np.concatenate([np.zeros((w - 1) // 2), f, np.zeros(w // 2)])
    ret = np.cumsum(padded)
    ret[w:] = ret[w:] - ret[:-w]
    mask = np.round(ret[w - 1:] / w).astype(bool)
    half = (VAD_MAX_SILENCE + 1) // 2
    out = np.zeros_like(mask)
    for o in range(-half, half + 1):                # a structuring element of seven ones about its centre
        lo, hi = max(0, o), min(mask.size, mask.size + o)
        if hi > lo:
            out[lo - o: hi - o] |= mask[lo: hi]
    return out


def tensor_specs() -> List[Tuple[str, Tuple[int, ...]]]:
    """(name, shape) of the encoder's tensors, torch's names: ``torch.nn.LSTM(40, 256, num_layers=3)`` and ``torch.nn.Linear(256, 256)``."""
    s: List[Tuple[str, Tuple[int, ...]]] = []
    for layer in range(LAYERS):
        kin = N_MELS if layer == 0 else HIDDEN
        s += [(f"lstm.weight_ih_l{layer}", (4 * HIDDEN, kin)), (f"lstm.weight_hh_l{layer}", (4 * HIDDEN, HIDDEN)),
              (f"lstm.bias_ih_l{layer}", (4 * HIDDEN,)), (f"lstm.bias_hh_l{layer}", (4 * HIDDEN,))]
    return s + [("linear.weight", (DIM, HIDDEN)), ("linear.bias", (DIM,))]


def synthetic_state(seed: int = 789) -> Dict[str, np.ndarray]:
    """Seeded float32 weights, uniform in +-1/16 = +-1/sqrt(256): torch's own initialisation scale for this LSTM."""
    rng = np.random.default_rng(int(seed))
    return {name: rng.uniform(-1.0 / 16.0, 1.0 / 16.0, size=shape).astype(np.float32) for name, shape in tensor_specs()}


def check_state(state: Dict[str, np.ndarray]) -> Dict[str, np.ndarray]:
    """The tensors of ``tensor_specs`` as contiguous float32 arrays; a missing name or a wrong shape is a ``ValueError``."""
    out = {}
    for name, shape in tensor_specs():
        if name not in state:
            raise ValueError(f"speaker encoder: tensor {name} is missing")
        a = np.ascontiguousarray(np.asarray(state[name]), dtype=np.float32)
        if a.shape != shape:
            raise ValueError(f"speaker encoder: tensor {name} has shape {a.shape}, expected {shape}")
        if not np.isfinite(a).all():
            raise ValueError(f"speaker encoder: tensor {name} holds values that are not finite")
        out[name] = a
    return out


def load(path: str) -> Dict[str, np.ndarray]:
    """The ``.npz`` tools/export_speaker_encoder.py writes (arrays only: ``allow_pickle=False``)."""
    if not str(path).lower().endswith(".npz"):
        raise ValueError(f"speaker encoder weights {path!r}: this package never unpickles a checkpoint.  Export it once with "
                         "`python tools/export_speaker_encoder.py IN.pt OUT.npz` and pass the .npz")
    with np.load(path, allow_pickle=False) as z:
        return check_state({k: z[k] for k in z.files})


def save(path: str, state: Dict[str, np.ndarray]) -> None:
    np.savez(path, **check_state(state))


# ------------------------------------------------------------------------------------------------ the embedder
class SpeakerEmbedder:
    """One ``rt_spk`` on the context (GPU, stream) of the engine whose output it embeds.  ``path``: the exported ``.npz``; without one
    the encoder runs on seeded weights only when ``synthetic=True``.  ``vad``: an optional callable ``(audio, sample_rate) -> flags``
    (one 0/1 flag per 480-sample window of the clip at 16 kHz, e.g. from webrtcvad) applied to every clip that comes without
    explicit ``voice_flags``; without it nothing is trimmed.  The instance is the ``embed`` of ``features.make_forest_scorer``."""

    dim = DIM

    def __init__(self, ctx: "_native.Context", path: Optional[str] = None, synthetic: bool = False,
                 vad: Optional[Callable[[torch.Tensor, int], Sequence[int]]] = None, seed: int = 789):
        if path is not None:
            state = load(path)
        elif synthetic:
            state = synthetic_state(seed)
        else:
            raise ValueError("no speaker encoder weights (path=None; this build cannot download resemblyzer's checkpoint): pass the .npz "
                             "written by tools/export_speaker_encoder.py, or synthetic=True for seeded weights")
        from .stt import hann_window, mel_filters
        self.ctx, self.lib, self.vad = ctx, ctx.lib, vad
        _declare(self.lib)
        h = C.c_void_p()
        ctx.check(self.lib.rt_spk_create(ctx.handle, C.byref(h)), "rt_spk_create")
        self.handle = h
        try:
            tensors = dict(check_state(state))
            tensors["mel.filters"] = mel_filters(N_FFT, N_MELS, SR)
            tensors["mel.window"] = hann_window(N_FFT)
            for name, a in tensors.items():
                a = np.ascontiguousarray(a, dtype=np.float32)
                rows, cols = (a.shape[0], 1) if a.ndim == 1 else a.shape
                ctx.check(self.lib.rt_spk_set_tensor(h, name.encode(), a.ctypes.data_as(C.POINTER(C.c_float)), rows, cols), f"rt_spk_set_tensor({name})")
            ctx.check(self.lib.rt_spk_finalize(h), "rt_spk_finalize")
        except Exception:
            self.close()
            raise

    def close(self) -> None:
        if getattr(self, "handle", None):
            self.lib.rt_spk_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _stage(self, audios: Sequence) -> List[torch.Tensor]:
        dev = torch.device(f"cuda:{self.ctx.device_ordinal}")
        xs = []
        for audio in audios:
            x = audio if isinstance(audio, torch.Tensor) else torch.as_tensor(np.asarray(audio, dtype=np.float32))
            x = x.detach().to(device=dev, dtype=torch.float32).reshape(-1).contiguous()
            if x.numel() < 1:
                raise ValueError("the speaker encoder needs at least one sample")
            xs.append(x)
        if xs:
            torch.cuda.current_stream(dev).synchronize()
        return xs

    def _flags(self, audios: Sequence, sample_rate: int, voice_flags) -> List[Optional[np.ndarray]]:
        if voice_flags is None:
            voice_flags = [None] * len(audios)
        if len(voice_flags) != len(audios):
            raise ValueError(f"{len(voice_flags)} sets of voice flags for {len(audios)} clips")
        out = []
        for audio, f in zip(audios, voice_flags):
            if f is None and self.vad is not None:
                f = self.vad(audio, sample_rate)
            out.append(None if f is None else np.ascontiguousarray(np.asarray(f).astype(bool).reshape(-1), dtype=np.uint8))
        return out

    def batch_partials(self, audios: Sequence, sample_rate: int, voice_flags=None) -> Tuple[np.ndarray, np.ndarray]:
        """(embeddings [n][256] float32, partial counts [n]) of a chunk of clips: one native call, one host synchronisation."""
        audios = list(audios)
        n = len(audios)
        if n == 0:
            return np.zeros((0, DIM), dtype=np.float32), np.zeros(0, dtype=np.int32)
        flags = self._flags(audios, sample_rate, voice_flags)
        xs = self._stage(audios)
        ptrs = (C.c_void_p * n)(*[x.data_ptr() for x in xs])
        lens = (C.c_int64 * n)(*[int(x.numel()) for x in xs])
        fptrs = (C.c_void_p * n)(*[None if f is None else f.ctypes.data for f in flags])
        fcnt = (C.c_int32 * n)(*[0 if f is None else int(f.size) for f in flags])
        emb = np.zeros((n, DIM), dtype=np.float32)
        parts = (C.c_int32 * n)()
        self.ctx.check(self.lib.rt_spk_embed_batch(self.handle, ptrs, lens, n, int(sample_rate), fptrs, fcnt, emb.ctypes.data_as(C.POINTER(C.c_float)), parts),
                       "rt_spk_embed_batch")
        return emb, np.array(parts, dtype=np.int32)

    def batch(self, audios: Sequence, sample_rate: int, voice_flags=None) -> np.ndarray:
        """Unit-norm embeddings [n][256] of a chunk of clips (the ``embed`` contract of ``make_forest_scorer``)."""
        return self.batch_partials(audios, sample_rate, voice_flags)[0]

    def __call__(self, audio, sample_rate: int):
        """A list or tuple of clips: ``batch``; one clip: its embedding [256], by the same path."""
        if isinstance(audio, (list, tuple)):
            return self.batch(audio, sample_rate)
        return self.batch([audio], sample_rate)[0]

    # ---- the stages on their own (tests)
    def debug_mel(self, audio, sample_rate: int, voice_flags=None) -> Tuple[np.ndarray, int]:
        """(mel [frames][40] of the preprocessed, zero-padded clip, its 16-kHz length after preprocessing)."""
        (x,) = self._stage([audio])
        f = None if voice_flags is None else np.ascontiguousarray(np.asarray(voice_flags).astype(bool).reshape(-1), dtype=np.uint8)
        n16 = -(-int(x.numel()) * SR // int(sample_rate)) if int(sample_rate) != SR else int(x.numel())
        cap = 2 + (n16 + PARTIAL_FRAMES * HOP) // HOP
        mel = np.zeros((cap, N_MELS), dtype=np.float32)
        nf, n_pre = C.c_int32(), C.c_int64()
        self.ctx.check(self.lib.rt_debug_spk_mel(self.handle, C.c_void_p(x.data_ptr()), x.numel(), int(sample_rate), None if f is None else f.ctypes.data,
                                                 0 if f is None else int(f.size), mel.ctypes.data_as(C.POINTER(C.c_float)), cap, C.byref(nf), C.byref(n_pre)),
                       "rt_debug_spk_mel")
        return mel[: nf.value], int(n_pre.value)

    def debug_lstm(self, partials: np.ndarray) -> np.ndarray:
        """Per-partial unit embeddings [P][256] of partials [P][160][40]."""
        p = np.ascontiguousarray(partials, dtype=np.float32)
        if p.ndim != 3 or p.shape[1:] != (PARTIAL_FRAMES, N_MELS):
            raise ValueError(f"partials of shape {p.shape}: expected [P][{PARTIAL_FRAMES}][{N_MELS}]")
        out = np.zeros((p.shape[0], DIM), dtype=np.float32)
        self.ctx.check(self.lib.rt_debug_spk_lstm(self.handle, p.ctypes.data_as(C.POINTER(C.c_float)), p.shape[0], out.ctypes.data_as(C.POINTER(C.c_float))),
                       "rt_debug_spk_lstm")
        return out
