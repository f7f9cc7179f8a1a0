"""Hand-crafted drift-classifier features on the GPU.

The reference's accent-drift classifier scores a 286-dimensional vector per segment (validation/classifier/trainer.py:23-68):
resemblyzer's 256-d speaker embedding + 13 MFCC means + 13 MFCC standard deviations + F0 mean / std (librosa.pyin) + the first two
LPC formants, all computed by librosa on a temporary WAV (base_tts.py:821-830).  This module produces the 30 hand-crafted
dimensions from the waveform in HBM: the per-sample work runs in csrc/features.hip behind ``rt_features_extract`` (resampler,
MFCC, the pYIN difference function, Burg LPC).  The single-clip path (``HandcraftedFeatures.__call__``) finishes pYIN here on the
host - trough statistics and Viterbi pass over the [frames][329] difference function - and these host functions are the
definition of the two kernels that do the same for a whole chunk of clips in one native call (``HandcraftedFeatures.batch``,
``rt_features_extract_batch``): there the host is left with the F0 statistics and the roots of one degree-18 polynomial per clip.
Natively the two calls are one path - the single-clip call is the batched one with one clip and without the two back-half kernels.

The 256-d embedding is produced by ``speaker.SpeakerEmbedder`` (csrc/speaker.hip: resemblyzer's GE2E encoder restated, parity
unpinned, weights from an exported ``.npz``), not here: an instance is the ``embed`` argument of ``make_forest_scorer``, which puts
its 256 dimensions in front of the 30.  The classifier itself is a pickled scikit-learn model this build will not load:
``make_drift_scorer`` takes it as a callable on the 30 dimensions (or on whatever vector the caller assembles around them);
``make_forest_scorer`` takes it as a ``forest.DriftForest`` - the same model exported to plain arrays, evaluated on the GPU for a
whole chunk in one call.

Definitions: librosa 0.10's defaults as the reference calls them, restated (oracle/features.py says which) - including the
reference's own quirk of leaving ``librosa.pyin``'s default ``sr=22050`` in place for 16-kHz audio, so that every F0 is
22050 / 16000 times the acoustic one.  Parity with librosa itself is UNPINNED (not installable here).
"""
from __future__ import annotations

import ctypes as C
import functools
import math
from typing import Callable, List, Optional, Sequence

import numpy as np
import torch

from . import _native

SR = 16000
PITCH_SR = 22050                                   # what librosa.pyin assumes when `sr` is not passed (trainer.py:52)
FMIN = 440.0 * 2.0 ** ((36 - 69) / 12.0)           # note_to_hz('C2')
FMAX = 440.0 * 2.0 ** ((96 - 69) / 12.0)           # note_to_hz('C7')
HOP = 512
BINS_PER_SEMITONE = 10                             # resolution 0.1
LPC_ORDER = max(12, SR // 1000 + 2)
N_THRESHOLDS, NO_TROUGH_PROB, SWITCH_PROB, MAX_TRANSITION_RATE = 100, 0.01, 0.01, 35.92

_DECLARED = False


def _declare(lib: C.CDLL) -> None:
    global _DECLARED
    if _DECLARED:
        return
    vp, i32, i64, pd = C.c_void_p, C.c_int32, C.c_int64, C.POINTER(C.c_double)
    lib.rt_features_create.argtypes = [vp, C.POINTER(vp)]
    lib.rt_features_destroy.argtypes = [vp]
    lib.rt_features_geometry.argtypes = [i32, C.c_double, C.c_double, C.POINTER(i32), C.POINTER(i32)]
    lib.rt_features_extract.argtypes = [vp, vp, i64, i32, i32, i32, i32, pd, C.POINTER(i32), pd, i32, C.POINTER(i32), pd]
    lib.rt_features_set_pitch_model.argtypes = [vp, i32, i32, i32, pd, pd, pd, pd, C.c_double, C.c_double, C.c_double, i32, C.c_double]
    lib.rt_features_extract_batch.argtypes = [vp, C.POINTER(vp), C.POINTER(i64), i32, i32, i32, i32, i32, pd, pd, C.POINTER(i32), i32, C.POINTER(i32)]
    lib.rt_debug_features_observe.argtypes = [vp, pd, i32, i32, i32, pd]
    lib.rt_debug_features_viterbi.argtypes = [vp, pd, C.POINTER(i32), i32, C.POINTER(i32), i32]
    _DECLARED = True


# ------------------------------------------------------------------------------------------------ pYIN, the host half
def _thresholds() -> np.ndarray:
    """The trough thresholds, ascending: the upper edges of N_THRESHOLDS equal bins of [0, 1]."""
    return np.linspace(0.0, 1.0, N_THRESHOLDS + 1)[1:]


def _beta_probs() -> np.ndarray:
    """Prior mass of each threshold bin under Beta(2, 18): I_x(2, 18) = 1 - (1 - x)^18 (1 + 18 x)."""
    x = np.linspace(0.0, 1.0, N_THRESHOLDS + 1)
    return np.diff(1.0 - (1.0 - x) ** 18 * (1.0 + 18.0 * x))


def default_n_bins() -> int:
    return int(math.floor(12 * BINS_PER_SEMITONE * math.log2(FMAX / FMIN))) + 1


def default_half_width() -> int:
    return (int(round(MAX_TRANSITION_RATE * 12 * HOP / PITCH_SR)) * BINS_PER_SEMITONE + 1) // 2


@functools.lru_cache(maxsize=4)
def _transition_tables(n_bins: int, hw: int):
    """What the Viterbi pass adds and compares, every transcendental evaluated here once (the one source of ``viterbi_banded`` and
    of the tables ``pitch_model`` uploads): ``srcc`` / ``ok`` [2 hw + 1][n_bins] = the from-bin of (offset, to-bin), clipped, and
    whether it exists; ``log_trans`` [2][2 hw + 1][n_bins] = log(w_local * p + tiny) for p = stay (0) / switch (1);
    ``log_init`` [2 n_bins] = log(p_init + tiny); ``neg`` = log(tiny), what the dense matrix holds outside the band.
    (Cached: callers read the arrays, nobody writes them.)"""
    tiny = np.finfo(np.float64).tiny
    j = np.arange(n_bins)
    # local[i][j] = (hw + 1 - |i - j|) / (hw + 1) / rowsum(i) for |i - j| <= hw
    lo_i, hi_i = np.maximum(0, j - hw), np.minimum(n_bins - 1, j + hw)
    tri = lambda d: (hw + 1.0 - np.abs(d)) / (hw + 1.0)                           # noqa: E731
    rowsum = np.array([tri(np.arange(lo_i[i], hi_i[i] + 1) - i).sum() for i in range(n_bins)])
    offs = np.arange(-hw, hw + 1)
    src = j[None, :] + offs[:, None]                                             # [offset][to] = from-bin
    ok = (src >= 0) & (src < n_bins)
    srcc = np.clip(src, 0, n_bins - 1)
    w_local = np.where(ok, tri(offs)[:, None] / rowsum[srcc], 0.0)               # local[from][to]
    log_trans = np.stack([np.log(w_local * (1.0 - SWITCH_PROB) + tiny), np.log(w_local * SWITCH_PROB + tiny)])
    p_init = np.zeros(2 * n_bins)
    p_init[n_bins:] = 1.0 / n_bins
    return srcc, ok, log_trans, np.log(p_init + tiny), np.log(tiny)


def pitch_model(n_bins: Optional[int] = None, hw: Optional[int] = None) -> dict:
    """The tables of pYIN's back half as ``rt_features_set_pitch_model`` takes them (float64, C order), built with the numpy
    expressions the host functions use: ``thresholds`` / ``beta`` [N_THRESHOLDS], ``log_trans`` [2][2 hw + 1][n_bins],
    ``log_init`` [2 n_bins], ``log_tiny``."""
    n_bins = default_n_bins() if n_bins is None else int(n_bins)
    hw = default_half_width() if hw is None else int(hw)
    _, _, log_trans, log_init, neg = _transition_tables(n_bins, hw)
    return {"n_bins": n_bins, "half_width": hw, "thresholds": np.ascontiguousarray(_thresholds()), "beta": np.ascontiguousarray(_beta_probs()),
            "log_trans": np.ascontiguousarray(log_trans), "log_init": np.ascontiguousarray(log_init), "log_tiny": float(neg)}


def observation_log_probs(cmnd: np.ndarray, min_period: int, n_bins: int) -> np.ndarray:
    """log of pyin's observation matrix, [frames][2 n_bins] (voiced pitch bins, then the unvoiced states), from the
    cumulative-mean-normalised difference function [frames][lags]: troughs, thresholds below each trough, Boltzmann(2) prior over
    the troughs under a threshold, Beta(2, 18) prior over the thresholds, parabolic refinement of the trough's lag."""
    T, n_lags = cmnd.shape
    thr = _thresholds()
    beta = _beta_probs()
    tiny = np.finfo(np.float64).tiny
    obs = np.zeros((T, 2 * n_bins))
    # parabolic shifts for every lag of every frame
    a = (cmnd[:, :-2] + cmnd[:, 2:] - 2.0 * cmnd[:, 1:-1]) / 2.0
    b = (cmnd[:, 2:] - cmnd[:, :-2]) / 2.0
    shifts = np.zeros_like(cmnd)
    shifts[:, 1:-1] = -b / (2.0 * a + tiny)
    shifts[np.abs(shifts) > 1.0] = 0.0
    trough = np.zeros_like(cmnd, dtype=bool)
    trough[:, 1:-1] = (cmnd[:, 1:-1] < cmnd[:, :-2]) & (cmnd[:, 1:-1] <= cmnd[:, 2:])
    trough[:, -1] = cmnd[:, -1] < cmnd[:, -2]
    trough[:, 0] = cmnd[:, 0] < cmnd[:, 1]
    e2 = math.exp(-2.0)
    for t in range(T):
        idx = np.flatnonzero(trough[t])
        if idx.size:
            h = cmnd[t, idx]
            below = h[:, None] < thr[None, :]                                   # [troughs][thresholds]
            n = below.sum(axis=0)
            pos = np.cumsum(below, axis=0) - 1
            with np.errstate(divide="ignore", invalid="ignore"):
                prior = np.where(below, (1.0 - e2) * np.exp(-2.0 * pos) / (1.0 - np.exp(-2.0 * np.maximum(n, 1)))[None, :], 0.0)
            probs = prior @ beta
            g = int(np.argmin(h))
            probs[g] += NO_TROUGH_PROB * float(beta[: int(np.count_nonzero(~below[g]))].sum())
            keep = probs != 0.0
            period = min_period + idx[keep] + shifts[t, idx[keep]]
            bins = np.clip(np.round(12 * BINS_PER_SEMITONE * np.log2((PITCH_SR / period) / FMIN)), 0, n_bins).astype(np.int64)
            obs[t, bins] = probs[keep]                                            # (ascending lag: a later trough in the same bin wins)
        voiced = min(1.0, max(0.0, float(obs[t, :n_bins].sum())))
        obs[t, n_bins:] = (1.0 - voiced) / n_bins
    return np.log(obs + tiny)


def viterbi_banded(log_obs: np.ndarray, n_bins: int, hw: Optional[int] = None) -> np.ndarray:
    """Most likely state path of pyin's HMM: 2 x n_bins states, pitch transitions a triangle over +-hw bins (row-normalised at the
    edges), voicing kept with probability 0.99.  The transition matrix is never formed: the best predecessor of (voicing v, bin j)
    is searched over the 2 x (2 hw + 1) states that can reach it, lowest state index first on ties (np.argmax's rule on the dense
    matrix, which oracle/features.py builds).  This is the definition of csrc/features.hip k_feat_viterbi."""
    T = log_obs.shape[0]
    srcc, ok, log_trans, log_init, neg = _transition_tables(n_bins, default_half_width() if hw is None else int(hw))
    j = np.arange(n_bins)
    S = 2 * n_bins
    ptr = np.zeros((T, S), dtype=np.int64)
    val = log_obs[0] + log_init
    for t in range(1, T):
        new = np.empty(S)
        for v_to in (0, 1):
            best = np.full(n_bins, -np.inf)
            arg = np.zeros(n_bins, dtype=np.int64)
            for v_from in (0, 1):                                                 # ascending state index: voiced block first
                lt = log_trans[0 if v_from == v_to else 1]
                cand = np.where(ok, val[v_from * n_bins + srcc] + lt, -np.inf)    # [offset][to]
                k = np.argmax(cand, axis=0)                                       # first maximum = lowest from-bin
                c = cand[k, j]
                take = c > best
                arg = np.where(take, v_from * n_bins + srcc[k, j], arg)
                best = np.where(take, c, best)
            # states outside the band reach (v_to, j) with log(tiny): they win only if everything inside is worse
            out_best = float(val.max()) + neg
            if np.any(out_best > best):
                dense_from = int(np.argmax(val))
                arg = np.where(out_best > best, dense_from, arg)
                best = np.maximum(best, out_best)
            new[v_to * n_bins: (v_to + 1) * n_bins] = log_obs[t, v_to * n_bins: (v_to + 1) * n_bins] + best
            ptr[t, v_to * n_bins: (v_to + 1) * n_bins] = arg
        val = new
    states = np.zeros(T, dtype=np.int64)
    states[-1] = int(np.argmax(val))
    for t in range(T - 2, -1, -1):
        states[t] = ptr[t + 1, states[t + 1]]
    return states


def f0_from_states(states: np.ndarray, n_bins: int) -> np.ndarray:
    """F0 per frame (NaN = unvoiced) of a state path: bin b of either voicing is FMIN 2^(b / (12 bins per semitone))."""
    states = np.asarray(states, dtype=np.int64)
    f0 = FMIN * 2.0 ** ((states % n_bins) / (12.0 * BINS_PER_SEMITONE))
    f0[states >= n_bins] = np.nan
    return f0


def f0_from_cmnd(cmnd: np.ndarray, min_period: int) -> np.ndarray:
    """F0 per frame (NaN = unvoiced) from the difference function: the back half of librosa.pyin."""
    n_bins = default_n_bins()
    states = viterbi_banded(observation_log_probs(np.asarray(cmnd, dtype=np.float64), min_period, n_bins), n_bins)
    return f0_from_states(states, n_bins)


def formants_from_lpc(a: np.ndarray):
    """(F1, F2): the two lowest root angles of the LPC polynomial between 90 Hz and sr / 4 (trainer.py:88-96)."""
    roots = np.roots(np.asarray(a, dtype=np.float64))
    roots = roots[roots.imag > 0]
    freqs = np.sort(np.angle(roots) * (SR / (2.0 * np.pi)))
    freqs = freqs[(freqs > 90) & (freqs < SR / 4)]
    return (float(freqs[0]) if freqs.size > 0 else 0.0), (float(freqs[1]) if freqs.size > 1 else 0.0)


# ------------------------------------------------------------------------------------------------ the extractor
class HandcraftedFeatures:
    """One ``rt_features`` on the context (GPU, stream) of the engine whose output it scores."""

    def __init__(self, ctx: "_native.Context"):
        self.ctx, self.lib = ctx, ctx.lib
        _declare(self.lib)
        h = C.c_void_p()
        ctx.check(self.lib.rt_features_create(ctx.handle, C.byref(h)), "rt_features_create")
        self.handle = h
        lo, hi = C.c_int32(), C.c_int32()
        if self.lib.rt_features_geometry(PITCH_SR, FMIN, FMAX, C.byref(lo), C.byref(hi)) != 0:
            raise ValueError("rt_features_geometry refused the pitch range")
        self.min_period, self.max_period = int(lo.value), int(hi.value)
        self.n_bins: Optional[int] = None                                         # set with the pitch model (batched path)

    def close(self) -> None:
        if getattr(self, "handle", None):
            self.lib.rt_features_destroy(self.handle)
            self.handle = None

    def _stage(self, audios: Sequence, sample_rate: int):
        """The clips as flat float32 tensors on the context's GPU, written (the current stream is synchronised), and room for the
        frames of the longest: what both native calls take."""
        dev = torch.device(f"cuda:{self.ctx.device_ordinal}")
        xs = []
        for audio in audios:
            x = audio if isinstance(audio, torch.Tensor) else torch.as_tensor(np.asarray(audio, dtype=np.float32))
            x = x.detach().to(device=dev, dtype=torch.float32).reshape(-1).contiguous()
            if x.numel() < 2:
                raise ValueError("feature extraction needs at least two samples")
            xs.append(x)
        if not xs:
            return xs, 0
        torch.cuda.current_stream(dev).synchronize()
        sr = int(sample_rate)
        return xs, 2 + max(-(-int(x.numel()) * SR // sr) if sr != SR else int(x.numel()) for x in xs) // HOP

    def raw(self, audio, sample_rate: int):
        """(mfcc mean+std [26], cmnd [frames][lags], lpc [order + 1]) - what comes off the GPU."""
        (x,), cap = self._stage([audio], sample_rate)
        n_lags = self.max_period - self.min_period + 1
        stats = (C.c_double * 26)()
        cmnd = np.zeros((cap, n_lags), dtype=np.float64)
        lpc = (C.c_double * (LPC_ORDER + 1))()
        nm, npf = C.c_int32(), C.c_int32()
        self.ctx.check(self.lib.rt_features_extract(self.handle, C.c_void_p(x.data_ptr()), x.numel(), int(sample_rate), self.min_period, self.max_period,
                                                    LPC_ORDER, stats, C.byref(nm), cmnd.ctypes.data_as(C.POINTER(C.c_double)), cap, C.byref(npf), lpc),
                       "rt_features_extract")
        return np.array(stats, dtype=np.float64), cmnd[: npf.value], np.array(lpc, dtype=np.float64)

    # ---- the batched path: one native call and one host synchronisation per chunk of clips, pYIN's back half on the device
    def set_pitch_model(self, model: Optional[dict] = None) -> None:
        """Upload the tables of pYIN's back half (``pitch_model()``; the real geometry unless a test hands in its own)."""
        m = pitch_model() if model is None else model
        pd = C.POINTER(C.c_double)
        arr = {k: np.ascontiguousarray(m[k], dtype=np.float64) for k in ("thresholds", "beta", "log_trans", "log_init")}
        if arr["log_trans"].shape != (2, 2 * m["half_width"] + 1, m["n_bins"]) or arr["log_init"].shape != (2 * m["n_bins"],) or \
                arr["thresholds"].shape != arr["beta"].shape:
            raise ValueError("pitch model tables do not have the shapes of pitch_model()")
        self.ctx.check(self.lib.rt_features_set_pitch_model(
            self.handle, int(m["n_bins"]), int(m["half_width"]), int(arr["thresholds"].shape[0]), arr["thresholds"].ctypes.data_as(pd),
            arr["beta"].ctypes.data_as(pd), arr["log_trans"].ctypes.data_as(pd), arr["log_init"].ctypes.data_as(pd), float(m["log_tiny"]),
            float(PITCH_SR), float(FMIN), int(BINS_PER_SEMITONE), float(NO_TROUGH_PROB)), "rt_features_set_pitch_model")
        self.n_bins = int(m["n_bins"])

    def _extract_batch(self, audios: Sequence, sample_rate: int):
        """(mfcc statistics [n][26], lpc [n][order + 1], state paths: n arrays of one state per pitch frame)."""
        if self.n_bins is None:
            self.set_pitch_model()
        xs, cap = self._stage(audios, sample_rate)
        n = len(xs)
        if n == 0:
            return np.zeros((0, 26)), np.zeros((0, LPC_ORDER + 1)), []
        ptrs = (C.c_void_p * n)(*[x.data_ptr() for x in xs])
        lens = (C.c_int64 * n)(*[int(x.numel()) for x in xs])
        stats = np.zeros((n, 26), dtype=np.float64)
        lpc = np.zeros((n, LPC_ORDER + 1), dtype=np.float64)
        states = np.zeros((n, cap), dtype=np.int32)
        npf = (C.c_int32 * n)()
        pd = C.POINTER(C.c_double)
        self.ctx.check(self.lib.rt_features_extract_batch(self.handle, ptrs, lens, n, int(sample_rate), self.min_period, self.max_period, LPC_ORDER,
                                                          stats.ctypes.data_as(pd), lpc.ctypes.data_as(pd), states.ctypes.data_as(C.POINTER(C.c_int32)),
                                                          cap, npf), "rt_features_extract_batch")
        return stats, lpc, [states[c, : npf[c]].astype(np.int64) for c in range(n)]

    def f0_states(self, audios: Sequence, sample_rate: int) -> List[np.ndarray]:
        """The Viterbi state path of every clip (voiced pitch bin b = state b, unvoiced = n_bins + b), decoded on the device."""
        return self._extract_batch(audios, sample_rate)[2]

    def batch(self, audios: Sequence, sample_rate: int) -> np.ndarray:
        """``__call__`` for a whole chunk of clips, [n][30]: one native call, one host synchronisation.  The state paths come from
        the device; the host finishes the F0 statistics and the formants of every clip."""
        stats, lpc, states = self._extract_batch(audios, sample_rate)
        out = np.zeros((len(states), 30), dtype=np.float64)
        for c, st in enumerate(states):
            f0 = f0_from_states(st, self.n_bins)
            v = f0[~np.isnan(f0)]
            f1, f2 = formants_from_lpc(lpc[c])
            out[c] = np.concatenate([stats[c], [float(v.mean()) if v.size else 0.0, float(v.std()) if v.size else 0.0, f1, f2]])
        return out

    def __call__(self, audio, sample_rate: int) -> np.ndarray:
        """[13 MFCC means | 13 MFCC stds | F0 mean | F0 std | F1 | F2] = elements 256..285 of the reference's feature vector."""
        stats, cmnd, lpc = self.raw(audio, sample_rate)
        f0 = f0_from_cmnd(cmnd, self.min_period)
        v = f0[~np.isnan(f0)]
        f1, f2 = formants_from_lpc(lpc)
        return np.concatenate([stats, [float(v.mean()) if v.size else 0.0, float(v.std()) if v.size else 0.0, f1, f2]])


def make_drift_scorer(extractor: HandcraftedFeatures, classifier: Callable[[np.ndarray], float],
                      embed: Optional[Callable[[torch.Tensor, int], np.ndarray]] = None) -> Callable[[torch.Tensor, int], float]:
    """A ``drift_scorer`` hook for the provider (provider.BatchedPipeline): ``(audio tensor, sample_rate) -> probability``.
    ``classifier`` maps the feature vector to the accent-drift probability (the reference's is a pickled scikit-learn model,
    ``predict_proba(...)[0, 1]``); ``embed`` optionally supplies the speaker-embedding dimensions that precede the hand-crafted ones
    in the reference's layout.  The callable carries ``score.batch(audios, sample_rate) -> list of probabilities``: the features of a
    whole chunk from one ``extractor.batch`` call, which the provider uses when it validates a chunk."""
    def score(audio: torch.Tensor, sample_rate: int) -> float:
        f = extractor(audio, sample_rate)
        if embed is not None:
            f = np.concatenate([np.asarray(embed(audio, sample_rate), dtype=np.float64).reshape(-1), f])
        return float(classifier(f))

    def batch(audios: Sequence[torch.Tensor], sample_rate: int) -> List[float]:
        out = []
        for audio, f in zip(audios, extractor.batch(audios, sample_rate)):
            if embed is not None:
                f = np.concatenate([np.asarray(embed(audio, sample_rate), dtype=np.float64).reshape(-1), f])
            out.append(float(classifier(f)))
        return out
    score.batch = batch
    return score


def forest_rows(extractor, embed, audios: Sequence, sample_rate: int, width: Optional[int] = None) -> np.ndarray:
    """The classifier's rows of a chunk of clips, float64 [n][k + 30]: ONE ``extractor.batch`` call for the 30 hand-crafted features
    and, with ``embed`` (a batch callable ``(audios, sample_rate) -> [n][k]``), one call for the speaker-embedding dimensions that come
    first in the reference's layout (trainer.py:61-65).  The one assembly behind inference (``make_forest_scorer``) and training
    (``forest_train.train``): a classifier is fitted on exactly the rows it will score.  ``width``: the row width a model expects,
    checked against what ``embed`` returned."""
    audios = list(audios)
    f = np.asarray(extractor.batch(audios, sample_rate), dtype=np.float64).reshape(len(audios), -1)
    if embed is not None:
        e = np.asarray(embed(audios, sample_rate), dtype=np.float64)
        if e.ndim != 2 or e.shape[0] != len(audios) or (width is not None and e.shape[1] + f.shape[1] != width):
            need = "" if width is None else (f": the classifier takes {width} features, {f.shape[1]} of them hand-crafted, so it needs "
                                             f"[{len(audios)}][{width - f.shape[1]}]")
            raise ValueError(f"embed returned an array of shape {e.shape} for {len(audios)} clips{need}")
        f = np.concatenate([e, f], axis=1)
    return f


def make_forest_scorer(extractor: HandcraftedFeatures, forest, embed: Optional[Callable[[Sequence[torch.Tensor], int], np.ndarray]] = None
                       ) -> Callable[[torch.Tensor, int], float]:
    """A ``drift_scorer`` hook whose classifier runs on the GPU too (forest.DriftForest): ``score.batch(audios, sample_rate)`` makes ONE
    ``extractor.batch`` call and then ONE ``forest.predict`` call for the whole chunk, and the single-clip form ``score(audio,
    sample_rate)`` is the same path with one row.  ``embed`` is a BATCH callable ``(audios, sample_rate) -> [n][k]`` for the
    speaker-embedding dimensions, which come first in the reference's layout (trainer.py:61-65): embedding, then the 30 hand-crafted
    features.  ``k + 30`` must be the forest's width, checked here: k is 0 without ``embed``, and ``embed.dim`` where the callable
    carries one; a callable without it can only be held to its width at its first call.  The ``ValueError`` names the sizes."""
    width = int(forest.n_features)
    if embed is None and width != 30:
        raise ValueError(f"the classifier takes {width} features, the extractor gives 30: {width - 30} embedding dimensions are needed (embed=...)")
    k = None if embed is None else getattr(embed, "dim", None)
    if embed is not None and (width <= 30 or (k is not None and int(k) + 30 != width)):
        raise ValueError(f"the classifier takes {width} features, the extractor gives 30 and the embedding {'some' if k is None else int(k)}: "
                         f"{width} != 30 + {'k' if k is None else int(k)}")

    def batch(audios: Sequence[torch.Tensor], sample_rate: int) -> List[float]:
        audios = list(audios)
        if not audios:
            return []
        return [float(p) for p in forest.predict(forest_rows(extractor, embed, audios, sample_rate, width))]

    def score(audio: torch.Tensor, sample_rate: int) -> float:
        return batch([audio], sample_rate)[0]
    score.batch = batch
    return score
