"""Reference of timestamp decoding and seek (rt_stt_transcribe_seek) in float64: a helper of the seek tests, not a test.

The two rules ("timestamps and seek").

The step rule, per decoder row, on the logits that remain after the suppress mask (from which the timestamp ids are exempt).  T0 is
the first timestamp id, T0 - 1 is <|notimestamps|>, h the row's generated history behind the forced prefix:
  * <|notimestamps|> never appears;
  * last token a timestamp and the one before it too (or len(h) < 2): no timestamp may follow;
  * last token a timestamp and the one before it not: nothing below end-of-sequence may follow;
  * timestamp ids in h: ids in [T0, last) are barred; last is the last timestamp when the row is closing a pair, else that + 1;
  * len(h) == 0: everything below T0 is barred, and with max_initial m >= 0 everything above T0 + m;
  * then, over the row as it stands: if logsumexp(timestamps) > max(text log-probability), everything below T0 is barred.
``step_bars`` is the first five points, ``step_row`` all six on one row of logits (what k_stt_beam_select<true> applies before it
ranks a row's candidates); both are held against transformers' WhisperTimeStampLogitsProcessor by tests/test_stt_seek_cpu.py.

The seek rule, per window, on the chosen hypothesis with end-of-sequence stripped (``seek_rule``; transformers' _retrieve_segment):
consecutive timestamp pairs close segments; with a single trailing timestamp the window is consumed whole; otherwise the tokens
behind the last closed pair are discarded and the next window starts at that pair's timestamp; without any pair the window is one
segment and is consumed whole.  A window that would advance by zero ticks advances by a whole window.

``window_search`` is beam search (tests/stt_beam_ref.py ``search``) under the step rule on transformers' Whisper as oracle/whisper.py
builds it; ``clip_transcribe`` is the seek loop over a clip.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Callable, List, Optional, Sequence, Tuple

import numpy as np
import torch

from tests import stt_beam_ref as R

INF = float("inf")


def suppress_mask(cfg) -> Tuple[np.ndarray, np.ndarray]:
    """(never, not-as-the-first-token) of the greedy rule with the timestamp ids taken out of `never`."""
    never, begin = R.masks(cfg)
    never = never.copy()
    never[cfg.timestamp_begin:cfg.timestamp_begin + cfg.n_timestamps] = False
    return never, begin


def step_bars(V: int, T0: int, eos: int, h: Sequence[int], max_initial: int = -1) -> np.ndarray:
    """The structural bars of one row (every point of the step rule but the last) as a boolean mask over the vocabulary."""
    bad = np.zeros(V, dtype=bool)
    bad[T0 - 1] = True
    h = [int(t) for t in h]
    last = len(h) >= 1 and h[-1] >= T0
    pen = len(h) < 2 or h[-2] >= T0
    if last:
        if pen:
            bad[T0:] = True
        else:
            bad[:eos] = True
    ts = [t for t in h if t >= T0]
    if ts:
        bad[T0:(ts[-1] if last and not pen else ts[-1] + 1)] = True
    if not h:
        bad[:T0] = True
        if max_initial >= 0:
            bad[T0 + max_initial + 1:] = True
    return bad


def state_of(h: Sequence[int], T0: int) -> Tuple[int, int]:
    """The per-row history state the device keeps: (flags, last timestamp id or 0); bit 0 of flags - the last token is a timestamp,
    bit 1 - the one before it is, or the history is shorter than two."""
    h = [int(t) for t in h]
    last = len(h) >= 1 and h[-1] >= T0
    pen = len(h) < 2 or h[-2] >= T0
    ts = [t for t in h if t >= T0]
    return (1 if last else 0) | (2 if pen else 0), (ts[-1] if ts else 0)


def bars_from_state(V: int, T0: int, NT: int, eos: int, flags: int, last_ts: int, first: bool, max_initial: int = -1) -> np.ndarray:
    """``step_bars`` as k_stt_beam_select<true> forms it, from the row's state alone: text ids are [text_lo, T0 - 1), timestamp ids
    [ts_lo, ts_hi), everything else is barred."""
    last, pen = bool(flags & 1), bool(flags & 2)
    text_lo, text_hi, ts_lo, ts_hi = 0, T0 - 1, T0, min(T0 + NT, V)
    if last_ts > 0:
        ts_lo = max(ts_lo, last_ts if last and not pen else last_ts + 1)
    if last and pen:
        ts_lo = ts_hi
    if last and not pen:
        text_lo = eos
    if first:
        text_lo = text_hi
        if max_initial >= 0:
            ts_hi = min(ts_hi, T0 + max_initial + 1)
    bad = np.ones(V, dtype=bool)
    bad[text_lo:text_hi] = False
    bad[ts_lo:ts_hi] = False
    return bad


def _lse(x: np.ndarray) -> float:
    x = x[np.isfinite(x)]
    if not x.size:
        return -INF
    m = x.max()
    return float(m + np.log(np.exp(x - m).sum()))


def step_row(logits, h: Sequence[int], T0: int, eos: int, never: np.ndarray, begin: Optional[np.ndarray], max_initial: int = -1) -> Tuple[np.ndarray, float]:
    """One row under the whole rule: the float64 logits with every barred id (and every NaN) at -inf, and the margin of the logsumexp
    decision, lse(timestamps) - max(text); text is barred when it is positive."""
    x = np.asarray(logits, dtype=np.float64).copy()
    bad = step_bars(x.size, T0, eos, h, max_initial) | never
    if not len(h) and begin is not None:
        bad = bad | begin
    x[bad | np.isnan(x)] = -INF
    lse_ts, max_text = _lse(x[T0:]), float(x[:T0].max())
    if lse_ts > max_text:
        x[:T0] = -INF
    if not np.isfinite(lse_ts) and not np.isfinite(max_text):
        return x, INF
    return x, lse_ts - max_text


def seek_rule(seq: Sequence[int], T0: int, own: int, whole: int) -> Tuple[List[Tuple[int, int, List[int]]], int]:
    """(segments, advance in ticks) of one window's hypothesis: a segment is (start tick, end tick, text ids), ticks of the window.
    own: the ticks the window's own samples span (the end of a segment nothing closes); whole: a whole window in ticks."""
    seq = [int(t) for t in seq]
    n = len(seq)
    ts = [t >= T0 for t in seq]
    text = lambda a, b: [t for t in seq[a:b] if t < T0]
    cuts = [k + 1 for k in range(n - 1) if ts[k] and ts[k + 1]]
    single = n >= 2 and not ts[-2] and ts[-1]
    segs: List[Tuple[int, int, List[int]]] = []
    if cuts:
        if single:
            cuts.append(n)
        else:
            cuts[-1] += 1
        last = 0
        for i, cur in enumerate(cuts):
            tail = i == len(cuts) - 1 and not single
            segs.append((seq[last] - T0, seq[cur - (2 if tail else 1)] - T0, text(last, cur)))
            last = cur
        adv = whole if single else seq[last - 2] - T0
    else:
        stamps = [t for t in seq if t >= T0]
        end = stamps[-1] - T0 if stamps and stamps[-1] != T0 else own
        segs.append((0, end, text(0, n)))
        adv = whole
    return segs, (adv if adv > 0 else whole)


@torch.no_grad()
def _logits(model, enc, prefix: Sequence[int], beams: List[List[int]]) -> np.ndarray:
    from transformers.modeling_outputs import BaseModelOutput
    ids = torch.tensor([[int(t) for t in prefix] + [int(t) for t in b] for b in beams])
    eo = BaseModelOutput(last_hidden_state=enc.expand(len(beams), -1, -1))
    return model(encoder_outputs=eo, decoder_input_ids=ids).logits[:, -1].double().numpy()


def ts_prefix(cfg, language: Optional[int] = None) -> List[int]:
    """The forced prefix of timestamp mode: the configuration's without its last entry (<|notimestamps|>), `language` at position 1."""
    p = [int(t) for t in cfg.prefix[:-1]]
    if language is not None and len(p) > 1:
        p[1] = int(language)
    return p


def budget_of(cfg) -> int:
    return min(int(cfg.max_new_tokens), cfg.n_text_ctx - (len(cfg.prefix) - 1))


@dataclass
class Window:
    offset: int                                  # input samples
    ids: List[int]                               # the hypothesis, timestamps included, end-of-sequence stripped
    logprob: float                               # its cumulative log-probability (end-of-sequence counted when it ended)
    count: int                                   # len(ids) + 1
    advance: int                                 # ticks
    segments: List[Tuple[int, int, List[int]]]   # ticks of the CLIP
    margin: float                                # the smallest margin of any decision the window rests on
    lse_margins: List[float] = field(default_factory=list)     # lse(timestamps) - max(text) of every row of every step
    no_speech_prob: float = float("nan")
    silent: bool = False


def window_search(model, cfg, mel: torch.Tensor, B: int, max_initial: int = -1, language: Optional[int] = None) -> Tuple[R.Result, List[float]]:
    """Beam search of width B (1: greedy) over one window's log-mel features under the step rule -> (result, lse margins)."""
    enc = R.encode(model, mel)
    never, begin = suppress_mask(cfg)
    prefix, T0, eos = ts_prefix(cfg, language), cfg.timestamp_begin, cfg.eos_id
    lse: List[float] = []

    def step_logits(beams):
        raw = _logits(model, enc, prefix, beams)
        out = np.empty_like(raw)
        for j, b in enumerate(beams):
            out[j], m = step_row(raw[j], b, T0, eos, never, begin, max_initial)
            lse.append(m)
        return out
    res = R.search(step_logits, B, budget_of(cfg), eos, np.zeros(cfg.vocab, dtype=bool), None)
    return res, lse


@torch.no_grad()
def rescore(model, cfg, mel: torch.Tensor, ids: Sequence[int], ended: bool, max_initial: int = -1, language: Optional[int] = None) -> float:
    """Teacher-forced cumulative log-probability of `ids` (timestamps included) under the step rule, and of end-of-sequence behind
    them if the hypothesis ended."""
    enc = R.encode(model, mel)
    never, begin = suppress_mask(cfg)
    prefix, T0, eos = ts_prefix(cfg, language), cfg.timestamp_begin, cfg.eos_id
    ids = [int(t) for t in ids]
    total = 0.0
    for k, t in enumerate(ids + ([eos] if ended else [])):
        x, _ = step_row(_logits(model, enc, prefix, [ids[:k]])[0], ids[:k], T0, eos, never, begin, max_initial)
        total += float(x[t] - _lse(x))
    return total


@dataclass
class Clip:
    ids: List[int]
    score: float
    segments: List[Tuple[int, int, List[int]]]   # ticks of the clip
    windows: List[Window]
    margin: float


def own_features(cfg, pcm: np.ndarray, sr: int) -> Callable[[int, int], torch.Tensor]:
    """A window's features from its own samples, as the native call takes them: resampled and featurised alone."""
    from oracle import whisper as OW

    def at(off: int, n: int) -> torch.Tensor:
        x = pcm[off:off + n]
        return OW.log_mel(cfg, OW.resample(x, sr, cfg.sample_rate) if sr != cfg.sample_rate else x)
    return at


def clip_transcribe(model, cfg, pcm: np.ndarray, sr: int, B: int = 1, max_initial: int = -1, language: Optional[int] = None,
                    no_speech_threshold: Optional[float] = None, logprob_threshold: Optional[float] = -1.0,
                    features: Optional[Callable[[int, int], torch.Tensor]] = None) -> Clip:
    """The seek loop over one clip.  Offsets in input samples, one tick = floor(0.02 sr) of them."""
    from rho_tts_amd.validation import window_is_silent
    from tests import stt_lang_ref as LR
    pcm = np.asarray(pcm, dtype=np.float32)
    features = features or own_features(cfg, pcm, sr)
    tick, win, whole = int(0.02 * sr), int(cfg.chunk_seconds) * sr, cfg.n_timestamps - 1
    off, wins, ids, segs = 0, [], [], []
    for _ in range(len(pcm) // tick + 2):
        n = min(win, len(pcm) - off)
        mel = features(off, n)
        res, lse = window_search(model, cfg, mel, B, max_initial, language)
        w = Window(off, list(res.ids), res.score, len(res.ids) + 1, whole, [], min([res.margin] + [abs(m) for m in lse]), lse)
        if no_speech_threshold is not None:
            w.no_speech_prob = float(np.exp(LR.detect(model, cfg, mel).log_no_speech_prob))
            w.silent = window_is_silent(w.no_speech_prob, w.logprob / w.count, no_speech_threshold, logprob_threshold)
        if not w.silent:
            local, w.advance = seek_rule(res.ids, cfg.timestamp_begin, min(whole, n // tick), whole)
            base = off // tick
            w.segments = [(base + a, base + b, t) for a, b, t in local]
            segs += w.segments
            ids += sum((t for _, _, t in local), [])
        wins.append(w)
        off += w.advance * tick
        if off >= len(pcm):
            break
    kept = [w for w in wins if not w.silent] or wins
    return Clip(ids, sum(w.logprob for w in kept) / sum(w.count for w in kept), segs, wins, min(w.margin for w in wins))
