"""The float64 oracle of the GE2E speaker encoder (rho_tts_amd/speaker.py, csrc/speaker.hip): resemblyzer 0.1.x's
``preprocess_wav`` + ``VoiceEncoder.embed_utterance`` restated in numpy / torch on the CPU, every stage on its own so that the tests
can hold each one.  Parity with resemblyzer itself is UNPINNED (neither it, webrtcvad nor librosa is installable here): this file is
the definition the kernels are held to.  It starts at the 16-kHz clip; the resampler in front of it is oracle/whisper.py's."""
from __future__ import annotations

import functools
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from rho_tts_amd import speaker as S
from rho_tts_amd.stt import hann_window, mel_filters


def normalize_volume(x: np.ndarray) -> np.ndarray:
    """normalize_volume(target -30 dBFS, increase_only=True) in float64; a clip of zeros is left unchanged."""
    x = np.asarray(x, dtype=np.float64)
    rms = np.sqrt(np.mean(x ** 2))
    if rms == 0.0:
        return x
    change = S.TARGET_DBFS - 20.0 * np.log10(rms)
    return x * 10.0 ** (change / 20.0) if change > 0.0 else x


def trim_long_silences(x: np.ndarray, flags) -> np.ndarray:
    """The clip cut to a multiple of 480 samples, its windows kept where the smoothed, dilated mask of ``flags`` is 1."""
    n_win = len(x) // S.VAD_WINDOW
    flags = np.asarray(flags).reshape(-1)
    assert flags.size == n_win
    mask = np.repeat(S.smooth_voice_flags(flags), S.VAD_WINDOW)
    return np.asarray(x)[: n_win * S.VAD_WINDOW][mask]


def preprocess(x16: np.ndarray, flags=None) -> np.ndarray:
    """Steps 2 and 3 on a 16-kHz float32 clip -> float32 (the kernels store the preprocessed clip in float32)."""
    y = normalize_volume(np.asarray(x16, dtype=np.float32))
    if flags is not None:
        y = trim_long_silences(y, flags)
    return y.astype(np.float32)


def mel(y: np.ndarray) -> np.ndarray:
    """[1 + n // 160][40] float64: librosa.feature.melspectrogram(y, sr=16000, n_fft=400, hop_length=160, n_mels=40).T with a
    zero-padded centre: periodic Hann, power spectrum, slaney filters, no log."""
    y = np.asarray(y, dtype=np.float64)
    n_frames = 1 + len(y) // S.HOP
    pad = np.concatenate([np.zeros(S.N_FFT // 2), y, np.zeros(S.N_FFT // 2)])
    idx = np.arange(n_frames)[:, None] * S.HOP + np.arange(S.N_FFT)[None, :]
    frames = pad[idx] * hann_window(S.N_FFT).astype(np.float64)[None, :]
    power = np.abs(np.fft.rfft(frames, axis=1)) ** 2
    return power @ mel_filters(S.N_FFT, S.N_MELS, S.SR).astype(np.float64)


def partials_of(y: np.ndarray) -> np.ndarray:
    """[P][160][40] float64: the partial utterances of the preprocessed clip (zero-padded to the last partial's end)."""
    slices, n_pad = S.partial_slices(len(y))
    m = mel(np.concatenate([np.asarray(y, dtype=np.float64), np.zeros(n_pad - len(y))]))
    return np.stack([m[a:b] for a, b in slices])


def sigmoid(v):
    return 1.0 / (1.0 + np.exp(-v))


def lstm_by_hand(state: Dict[str, np.ndarray], x: np.ndarray) -> np.ndarray:
    """h_T of the top layer, [P][256] float64, from the step equations written out: gates i, f, g, o in that order along the 1024
    rows, both biases added, zero initial state.  (tests/test_speaker_embed_cpu.py holds it to torch.nn.LSTM.)"""
    seq = np.asarray(x, dtype=np.float64)
    H = S.HIDDEN
    for layer in range(S.LAYERS):
        w_ih, w_hh = (state[f"lstm.weight_{k}_l{layer}"].astype(np.float64) for k in ("ih", "hh"))
        b = state[f"lstm.bias_ih_l{layer}"].astype(np.float64) + state[f"lstm.bias_hh_l{layer}"].astype(np.float64)
        h, c = np.zeros((seq.shape[0], H)), np.zeros((seq.shape[0], H))
        out = np.zeros((seq.shape[0], seq.shape[1], H))
        for t in range(seq.shape[1]):
            g = seq[:, t] @ w_ih.T + h @ w_hh.T + b
            i, f, gg, o = sigmoid(g[:, :H]), sigmoid(g[:, H: 2 * H]), np.tanh(g[:, 2 * H: 3 * H]), sigmoid(g[:, 3 * H:])
            c = f * c + i * gg
            h = o * np.tanh(c)
            out[:, t] = h
        seq = out
    return seq[:, -1]


def torch_lstm(state: Dict[str, np.ndarray], dtype=torch.float64) -> torch.nn.LSTM:
    net = torch.nn.LSTM(S.N_MELS, S.HIDDEN, num_layers=S.LAYERS, batch_first=True)
    net.load_state_dict({k[len("lstm."):]: torch.from_numpy(np.array(v)) for k, v in state.items() if k.startswith("lstm.")})
    return net.to(dtype).eval()


def partial_embeds(state: Dict[str, np.ndarray], parts: np.ndarray, dtype=torch.float64) -> np.ndarray:
    """[P][256]: relu(W h_T + b) / norm per partial, the network in ``dtype`` (float64: the oracle; float32: torch's own error)."""
    with torch.no_grad():
        _, (h, _) = torch_lstm(state, dtype)(torch.from_numpy(np.ascontiguousarray(parts)).to(dtype))
        w, b = torch.tensor(state["linear.weight"], dtype=dtype), torch.tensor(state["linear.bias"], dtype=dtype)
        e = torch.relu(h[-1] @ w.T + b)
        norm = e.norm(dim=1, keepdim=True)
        e = torch.where(norm > 0, e / norm.clamp_min(1e-300), torch.zeros_like(e))
    return e.to(torch.float64).numpy()


def utterance(pe: np.ndarray) -> np.ndarray:
    m = np.asarray(pe, dtype=np.float64).mean(axis=0)
    norm = np.linalg.norm(m)
    return m / norm if norm > 0 else np.zeros_like(m)


def embed(state: Dict[str, np.ndarray], x16: np.ndarray, flags=None) -> Tuple[np.ndarray, int]:
    """(unit embedding [256] float64, number of partials) of a 16-kHz clip: steps 2 - 7."""
    parts = partials_of(preprocess(x16, flags))
    return utterance(partial_embeds(state, parts)), parts.shape[0]


@functools.lru_cache(maxsize=None)
def state(seed: int = 789) -> Dict[str, np.ndarray]:
    """The seeded weights the GPU tests run on (read-only, shared)."""
    st = S.synthetic_state(seed)
    for a in st.values():
        a.setflags(write=False)
    return st
