"""Reference of sampled decoding and the temperature fallback (rt_stt_set_fallback) in float64: a helper of the fallback tests, not a test.

The rule ("temperature fallback").

The generator.  ``row_hash`` is the mix32 chain of rt_uniform (oracle/sampling.py) over (seed, window key, temperature index, sample
index, step); per id, k = mix32(row_hash + id * 0x85EBCA77) >> 9 - the top 23 bits - u = (k + 0.5) 2^-23 and g = -log(-log(u)).  u is
exact in float32 and in float64, and lies in [2^-24, 1 - 2^-24]; g here is float64 from that exact u.

The sampled step, on one row at temperature T > 0: the row is masked as for a beam step (``stt_beam_ref.log_softmax``'s mask, or the
whole timestamp rule, ``stt_seek_ref.step_row``) on the UNTEMPERED logits, its log-probabilities are their log-softmax, and the pick is
the arg-max of x / T + g over the surviving ids, the lower id on ties (Gumbel-max: the pick is distributed as softmax(x / T)).  The
row's score adds the untempered log-probability of the pick; end-of-sequence ends the row.

A window at T > 0 is ``best_of`` rows with sample index 0 .. best_of - 1; its result is the row with the largest score / (ids + 1), the
lower index on ties.  ``fallback`` is the loop over the temperatures on one window (validation.needs_fallback / pick_attempt).
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Callable, List, Optional, Sequence, Tuple

import numpy as np
import torch

from rho_tts_amd.validation import needs_fallback, pick_attempt
from tests import stt_beam_ref as R
from tests import stt_seek_ref as SR

INF = float("inf")
M32 = 0xFFFFFFFF


def mix32(h):
    """murmur3's fmix32 on uint64 arrays (or ints) holding values < 2^32."""
    h = np.asarray(h, dtype=np.uint64) & np.uint64(M32)
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x85EBCA6B)) & np.uint64(M32)
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(0xC2B2AE35)) & np.uint64(M32)
    h ^= h >> np.uint64(16)
    return h


def row_hash(seed: int, key: int, t_index: int, sample: int, step: int) -> int:
    a = int(mix32((seed & M32) ^ 0x85EBCA6B))
    b = int(mix32((a + (key & M32) * 0x9E3779B1) & M32))
    c = int(mix32((b + t_index * 0x85EBCA77) & M32))
    d = int(mix32((c + sample * 0xC2B2AE3D + ((seed >> 32) & M32)) & M32))
    return int(mix32((d + step * 0x9E3779B1) & M32))


def counter_k(rh, ids) -> np.ndarray:
    """The 23-bit counter of every id under row hash(es) ``rh`` (broadcast against ``ids``)."""
    ids = np.asarray(ids, dtype=np.uint64)
    rh = np.asarray(rh, dtype=np.uint64)
    return (mix32((rh + ids * np.uint64(0x85EBCA77)) & np.uint64(M32)) >> np.uint64(9)).astype(np.int64)


def u_of_k(k) -> np.ndarray:
    return (np.asarray(k, dtype=np.float64) + 0.5) * 2.0 ** -23


def gumbel(rh, ids) -> np.ndarray:
    return -np.log(-np.log(u_of_k(counter_k(rh, ids))))


@dataclass
class Pick:
    tok: int                 # the pick (-1: the row has no survivor)
    lp: float                # its untempered log-probability
    val: float               # the winning perturbed value
    gap: float               # winning value - the runner-up's (inf: a single survivor)


def pick_masked(x: np.ndarray, T: float, rh) -> Pick:
    """The sampled step on a row already masked: ``x`` float64 with every barred id (and NaN) at -inf."""
    alive = np.flatnonzero(np.isfinite(x))
    if not alive.size:
        return Pick(-1, 0.0, -INF, INF)
    v = x[alive] / T + gumbel(rh, alive)
    order = np.lexsort((alive, -v))
    tok = int(alive[order[0]])
    m = x[alive].max()
    lse = m + np.log(np.exp(x[alive] - m).sum())
    return Pick(tok, float(x[tok] - lse), float(v[order[0]]), float(v[order[0]] - v[order[1]]) if alive.size > 1 else INF)


def sample_row(logits, bad: np.ndarray, T: float, rh) -> Pick:
    """Without the timestamp rule: ``bad`` the ids the masks bar at this step."""
    x = np.asarray(logits, dtype=np.float64).copy()
    x[bad | np.isnan(x)] = -INF
    return pick_masked(x, T, rh)


def sample_row_ts(logits, h: Sequence[int], T0: int, eos: int, never: np.ndarray, begin: Optional[np.ndarray], max_initial: int, T: float, rh) -> Tuple[Pick, float]:
    """Under the timestamp rule: (pick, margin of the logsumexp decision)."""
    x, m = SR.step_row(logits, h, T0, eos, never, begin, max_initial)
    return pick_masked(x, T, rh), m


@dataclass
class Sampled:
    ids: List[int]
    score: float
    ended: bool
    gap: float               # the smallest gap of any of its picks
    lse_margin: float = INF  # the smallest |lse(timestamps) - max(text)| of its steps (timestamp mode)


def sample_sequence(step_logits: Callable[[List[int]], np.ndarray], pick_row: Callable[[np.ndarray, List[int], int], Tuple[Pick, float]], budget: int, eos: int) -> Sampled:
    """One sampled row: step_logits(ids) -> the row's raw logits behind prefix + ids; pick_row(logits, ids, step) -> (Pick, lse margin)."""
    ids: List[int] = []
    score, gap, lse = 0.0, INF, INF
    for step in range(budget):
        p, m = pick_row(step_logits(ids), ids, step)
        gap, lse = min(gap, p.gap), min(lse, abs(m))
        if p.tok < 0:
            return Sampled(ids, score, True, gap, lse)
        score += p.lp
        if p.tok == eos:
            return Sampled(ids, score, True, gap, lse)
        ids = ids + [p.tok]
    return Sampled(ids, score, False, gap, lse)


def best_of(rows: Sequence[Sampled]) -> Tuple[int, float]:
    """(index of the row with the largest score / (ids + 1), the lower index on ties; its margin over the runner-up)."""
    norms = [r.score / (len(r.ids) + 1) for r in rows]
    best = int(np.argmax(norms))
    return best, min([norms[best] - n for k, n in enumerate(norms) if k != best] or [INF])


@dataclass
class Attempt:
    ids: List[int]           # timestamps included in timestamp mode
    score: float
    temperature: float
    ratio: Optional[float]
    avg: float
    margin: float            # the smallest margin of what the attempt rests on: the beam search's, or the best-of choice's
    gap: float = INF         # the smallest pick gap of any of its rows (sampled attempts)
    lse_margin: float = INF


@dataclass
class Fallback:
    chosen: int
    attempts: List[Attempt] = field(default_factory=list)
    threshold_margin: float = INF     # the smallest |avg - logprob_threshold| over the attempts (inf: the threshold is off)
    pick_margin: float = INF          # all failed: the chosen average - the runner-up's among the pool

    @property
    def result(self) -> Attempt:
        return self.attempts[self.chosen]


def fallback(decode_beam: Callable[[], Attempt], decode_sampled: Callable[[float, int], Attempt], temperatures: Sequence[float], text_ids: Callable[[List[int]], List[int]],
             ratio: Optional[Callable[[List[int]], float]], no_speech_prob: float = float("nan"), compression_ratio_threshold: Optional[float] = 2.4,
             logprob_threshold: Optional[float] = -1.0, no_speech_threshold: Optional[float] = None) -> Fallback:
    """The loop on one window.  decode_beam() is the temperature-0 attempt, decode_sampled(T, t_index) an attempt at T > 0; ``ratio`` is
    asked for the attempt's text ids (not asked, and 0, when there are none), as the native loop asks its callback."""
    out = Fallback(-1)
    for t, T in enumerate(temperatures):
        a = decode_beam() if T == 0 else decode_sampled(float(T), t)
        a.temperature, a.avg = float(T), a.score / (len(a.ids) + 1)
        if ratio is not None:
            txt = text_ids(a.ids)
            a.ratio = float(ratio(txt)) if txt else 0.0
        out.attempts.append(a)
        if logprob_threshold is not None:
            out.threshold_margin = min(out.threshold_margin, abs(a.avg - logprob_threshold))
        if not needs_fallback(a.ratio, a.avg, no_speech_prob, compression_ratio_threshold, logprob_threshold, no_speech_threshold):
            out.chosen = len(out.attempts) - 1
            return out
    pairs = [(a.ratio, a.avg) for a in out.attempts]
    out.chosen = pick_attempt(pairs, compression_ratio_threshold)
    within = [k for k, (r, _) in enumerate(pairs) if compression_ratio_threshold is None or r is None or not r > compression_ratio_threshold] or list(range(len(pairs)))
    out.pick_margin = min([pairs[out.chosen][1] - pairs[k][1] for k in within if k != out.chosen] or [INF])
    return out


# ---------------------------------------------------------------------------------------------- on the oracle model
@torch.no_grad()
def _logits(model, enc, prefix: Sequence[int], ids: List[int]) -> np.ndarray:
    return SR._logits(model, enc, prefix, [ids])[0]


def window_sampled(model, cfg, mel: torch.Tensor, S: int, T: float, seed: int, key: int, t_index: int, timestamps: bool = False, max_initial: int = -1,
                   language: Optional[int] = None) -> Attempt:
    """A window at temperature T: S sampled rows on transformers' Whisper as oracle/whisper.py builds it, and the best of them."""
    enc = R.encode(model, mel)
    eos = cfg.eos_id
    if timestamps:
        never, begin = SR.suppress_mask(cfg)
        prefix, budget, T0 = SR.ts_prefix(cfg, language), SR.budget_of(cfg), cfg.timestamp_begin
    else:
        never, begin = R.masks(cfg)
        prefix, budget = [int(t) for t in cfg.prefix], R.budget_of(cfg)
        if language is not None and len(prefix) > 1:
            prefix[1] = int(language)
    rows = []
    for j in range(S):
        def pick_row(lg, ids, step, j=j):
            rh = row_hash(seed, key, t_index, j, step)
            if timestamps:
                return sample_row_ts(lg, ids, T0, eos, never, begin, max_initial, T, rh)
            return sample_row(lg, (never | begin) if step == 0 else never, T, rh), INF
        rows.append(sample_sequence(lambda ids: _logits(model, enc, prefix, ids), pick_row, budget, eos))
    best, margin = best_of(rows)
    r = rows[best]
    return Attempt(list(r.ids), r.score, T, None, 0.0, margin, min(x.gap for x in rows), min(x.lse_margin for x in rows))


def window_beam(model, cfg, mel: torch.Tensor, B: int, timestamps: bool = False, max_initial: int = -1, language: Optional[int] = None) -> Attempt:
    if timestamps:
        res, lse = SR.window_search(model, cfg, mel, B, max_initial, language)
        return Attempt(list(res.ids), res.score, 0.0, None, 0.0, res.margin, INF, min([abs(m) for m in lse] or [INF]))
    res = R.beam_search(model, cfg, mel, B)
    return Attempt(list(res.ids), res.score, 0.0, None, 0.0, res.margin)


def window_fallback(model, cfg, mel: torch.Tensor, B: int, S: int, temperatures: Sequence[float], seed: int, key: int, ratio=None, timestamps: bool = False,
                    max_initial: int = -1, language: Optional[int] = None, no_speech_prob: float = float("nan"), compression_ratio_threshold: Optional[float] = 2.4,
                    logprob_threshold: Optional[float] = -1.0, no_speech_threshold: Optional[float] = None) -> Fallback:
    T0 = cfg.timestamp_begin if timestamps else None
    return fallback(lambda: window_beam(model, cfg, mel, B, timestamps, max_initial, language),
                    lambda T, t: window_sampled(model, cfg, mel, S, T, seed, key, t, timestamps, max_initial, language), temperatures,
                    (lambda ids: [i for i in ids if i < T0]) if timestamps else (lambda ids: list(ids)), ratio, no_speech_prob,
                    compression_ratio_threshold, logprob_threshold, no_speech_threshold)


def decisive(fb: Fallback, E: float, G: float, MARGIN: float) -> bool:
    """Whether a device whose logits are off by E and whose Gumbel term by G decides every step of ``fb`` as the reference does."""
    for a in fb.attempts:
        if a.margin < MARGIN or a.lse_margin < MARGIN:
            return False
        if a.temperature > 0 and a.gap < 4 * (E / a.temperature + G):
            return False
    return fb.threshold_margin >= MARGIN and fb.pick_margin >= MARGIN


def script(groups: Sequence[Sequence[int]], n_temperatures: int, high: float = 9.0, low: float = 1.0) -> List[float]:
    """The returns of a scripted ratio callback, in call order: per group of windows (in the order the call decodes them), window w's
    first ``groups[g][w]`` attempts get ``high`` and the next ``low``.  Per attempt the loop asks for the windows that still need one."""
    out: List[float] = []
    for ks in groups:
        need = list(range(len(ks)))
        for t in range(n_temperatures):
            out += [high if t < ks[w] else low for w in need]
            need = [w for w in need if t < ks[w]]
            if not need:
                break
    return out


@dataclass
class SeekWindow:
    offset: int
    fb: Fallback
    advance: int
    segments: List[Tuple[int, int, List[int]]]   # ticks of the clip


def clip_fallback_seek(model, cfg, pcm: np.ndarray, sr: int, B: int, S: int, temperatures: Sequence[float], seed: int, ratio=None, max_initial: int = -1,
                       compression_ratio_threshold: Optional[float] = 2.4, logprob_threshold: Optional[float] = -1.0) -> List[SeekWindow]:
    """The seek loop (tests/stt_seek_ref.py clip_transcribe, no silence rule) with the fallback loop on every window: the window key is
    the window's start in ticks, and the seek rule sees the chosen attempt."""
    pcm = np.asarray(pcm, dtype=np.float32)
    features = SR.own_features(cfg, pcm, sr)
    tick, win, whole = int(0.02 * sr), int(cfg.chunk_seconds) * sr, cfg.n_timestamps - 1
    off, wins = 0, []
    for _ in range(len(pcm) // tick + 2):
        n = min(win, len(pcm) - off)
        fb = window_fallback(model, cfg, features(off, n), B, S, temperatures, seed, off // tick, ratio, True, max_initial, None, float("nan"),
                             compression_ratio_threshold, logprob_threshold)
        local, adv = SR.seek_rule(fb.result.ids, cfg.timestamp_begin, min(whole, n // tick), whole)
        base = off // tick
        wins.append(SeekWindow(off, fb, adv, [(base + a, base + b, t) for a, b, t in local]))
        off += adv * tick
        if off >= len(pcm):
            break
    return wins
