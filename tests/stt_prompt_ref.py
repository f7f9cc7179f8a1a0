"""Reference of conditioning on previous text (rt_stt_set_prompt) in float64: a helper of the prompt tests, not a test.

The rule ("conditioning on previous text"; faster-whisper's ``transcribe`` / ``get_prompt``, restated).  A clip
has a history of ids - it starts as the initial prompt - and a reset mark.  A window's prompt is the history behind the mark, cut to
its last n_text_ctx / 2 - 1 ids (validation.prompt_for_window); with a prompt the window decodes behind
[sot_prev] + prompt + the timestamp-mode prefix, without one behind that prefix alone, in every attempt of a fallback policy; its
budget is min(max_new_tokens, n_text_ctx - the prefix' length).  The step rule's "generated history" starts behind the whole prefix:
prompt ids are not scored and are no part of h.  After a window that is not silent the history gains the ids of its closed segments,
timestamps included (``raw_slices``: the slices the seek rule cuts; a discarded tail is none of them), but for segments of no duration
or without a text id, and the mark moves to the end when conditioning is off or the chosen attempt ran above the reset temperature
(validation.history_after_window).

The step rule, the beam search and the seek rule are those of tests/stt_seek_ref.py and tests/stt_beam_ref.py; the sampled attempts
and the fallback loop those of tests/stt_sample_ref.py.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Callable, List, Optional, Sequence, Tuple

import numpy as np

from rho_tts_amd.validation import history_after_window, prompt_for_window, window_is_silent
from tests import stt_beam_ref as R
from tests import stt_sample_ref as PR
from tests import stt_seek_ref as SR

INF = float("inf")


def prompt_cap(cfg) -> int:
    return cfg.n_text_ctx // 2 - 1


def window_prefix(cfg, sot_prev: int, prompt: Sequence[int], language: Optional[int] = None) -> List[int]:
    """What a window decodes behind: the language stays at position 1 of the forced part."""
    forced = SR.ts_prefix(cfg, language)
    return ([int(sot_prev)] + [int(t) for t in prompt] + forced) if len(prompt) else forced


def budget_of(cfg, prefix: Sequence[int]) -> int:
    return min(int(cfg.max_new_tokens), cfg.n_text_ctx - len(prefix))


def raw_slices(seq: Sequence[int], T0: int, own: int, whole: int) -> List[Tuple[int, int, List[int], List[int]]]:
    """The closed segments of one window's hypothesis as (start tick, end tick, text ids, every id of the slice): the cuts of
    ``stt_seek_ref.seek_rule``, with what each slice holds beside its text."""
    seq = [int(t) for t in seq]
    n = len(seq)
    ts = [t >= T0 for t in seq]
    cuts = [k + 1 for k in range(n - 1) if ts[k] and ts[k + 1]]
    single = n >= 2 and not ts[-2] and ts[-1]
    out = []
    if cuts:
        if single:
            cuts.append(n)
        else:
            cuts[-1] += 1
        last = 0
        for i, cur in enumerate(cuts):
            tail = i == len(cuts) - 1 and not single
            out.append((seq[last] - T0, seq[cur - (2 if tail else 1)] - T0, [t for t in seq[last:cur] if t < T0], seq[last:cur]))
            last = cur
    else:
        stamps = [t for t in seq if t >= T0]
        out.append((0, stamps[-1] - T0 if stamps and stamps[-1] != T0 else own, [t for t in seq if t < T0], list(seq)))
    segs, _ = SR.seek_rule(seq, T0, own, whole)
    assert [(a, b, t) for a, b, t, _ in out] == [(a, b, t) for a, b, t in segs]
    return out


def window_search(model, cfg, enc, prefix: Sequence[int], B: int, max_initial: int = -1) -> Tuple[R.Result, List[float]]:
    """``stt_seek_ref.window_search`` behind any prefix, with the budget that prefix leaves."""
    never, begin = SR.suppress_mask(cfg)
    T0, eos = cfg.timestamp_begin, cfg.eos_id
    lse: List[float] = []

    def step_logits(beams):
        raw = SR._logits(model, enc, prefix, beams)
        out = np.empty_like(raw)
        for j, b in enumerate(beams):
            out[j], m = SR.step_row(raw[j], b, T0, eos, never, begin, max_initial)
            lse.append(m)
        return out
    return R.search(step_logits, B, budget_of(cfg, prefix), eos, np.zeros(cfg.vocab, dtype=bool), None), lse


def window_beam(model, cfg, enc, prefix, B: int, max_initial: int = -1) -> PR.Attempt:
    res, lse = window_search(model, cfg, enc, prefix, B, max_initial)
    return PR.Attempt(list(res.ids), res.score, 0.0, None, 0.0, res.margin, INF, min([abs(m) for m in lse] or [INF]))


def window_sampled(model, cfg, enc, prefix, S: int, T: float, seed: int, key: int, t_index: int, max_initial: int = -1) -> PR.Attempt:
    """``stt_sample_ref.window_sampled`` in timestamp mode behind any prefix."""
    never, begin = SR.suppress_mask(cfg)
    T0, eos = cfg.timestamp_begin, cfg.eos_id
    rows = []
    for j in range(S):
        def pick_row(lg, ids, step, j=j):
            return PR.sample_row_ts(lg, ids, T0, eos, never, begin, max_initial, T, PR.row_hash(seed, key, t_index, j, step))
        rows.append(PR.sample_sequence(lambda ids: SR._logits(model, enc, prefix, [ids])[0], pick_row, budget_of(cfg, prefix), eos))
    best, margin = PR.best_of(rows)
    r = rows[best]
    return PR.Attempt(list(r.ids), r.score, T, None, 0.0, margin, min(x.gap for x in rows), min(x.lse_margin for x in rows))


@dataclass
class Window:
    offset: int
    prompt: List[int]
    ids: List[int]
    logprob: float
    advance: int
    segments: List[Tuple[int, int, List[int]]]   # ticks of the clip
    slices: List[Tuple[int, int, List[int], List[int]]]
    reset: bool
    margin: float
    temperature: float = 0.0
    fb: Optional[PR.Fallback] = None
    silent: bool = False
    budget: int = 0


@dataclass
class Clip:
    ids: List[int]
    score: float
    segments: List[Tuple[int, int, List[int]]]
    windows: List[Window]
    margin: float
    history: List[int] = field(default_factory=list)


@dataclass
class Policy:
    """A fallback policy for ``clip_transcribe``: ``ratio`` is asked once per attempt, in the order the loop makes them."""
    temperatures: Sequence[float]
    best_of: int
    seed: int
    ratio: Optional[Callable[[List[int]], float]] = None
    compression_ratio_threshold: Optional[float] = 2.4
    logprob_threshold: Optional[float] = -1.0


def clip_transcribe(model, cfg, pcm: np.ndarray, sr: int, B: int, sot_prev: int, max_initial: int = -1, condition: bool = True, initial: Sequence[int] = (),
                    reset_on_temperature: Optional[float] = 0.5, language: Optional[int] = None, policy: Optional[Policy] = None,
                    no_speech_threshold: Optional[float] = None, logprob_threshold: Optional[float] = -1.0) -> Clip:
    """The seek loop of tests/stt_seek_ref.py over one clip under a prompt policy (and, ``policy``, the fallback loop on every window)."""
    from tests import stt_lang_ref as LR
    pcm = np.asarray(pcm, dtype=np.float32)
    features = SR.own_features(cfg, pcm, sr)
    tick, win, whole = int(0.02 * sr), int(cfg.chunk_seconds) * sr, cfg.n_timestamps - 1
    T0 = cfg.timestamp_begin
    history, mark = [int(t) for t in initial], 0
    off, wins, ids, segs = 0, [], [], []
    for _ in range(len(pcm) // tick + 2):
        n = min(win, len(pcm) - off)
        mel = features(off, n)
        enc = R.encode(model, mel)
        prompt = prompt_for_window(history, mark, prompt_cap(cfg))
        prefix = window_prefix(cfg, sot_prev, prompt, language)
        fb = None
        if policy is None:
            a = window_beam(model, cfg, enc, prefix, B, max_initial)
        else:
            fb = PR.fallback(lambda: window_beam(model, cfg, enc, prefix, B, max_initial),
                             lambda T, t: window_sampled(model, cfg, enc, prefix, policy.best_of, T, policy.seed, off // tick, t, max_initial),
                             policy.temperatures, lambda x: [i for i in x if i < T0], policy.ratio, float("nan"), policy.compression_ratio_threshold,
                             policy.logprob_threshold)
            a = fb.result
        w = Window(off, prompt, list(a.ids), a.score, whole, [], [], False, min(a.margin, a.lse_margin), a.temperature, fb, budget=budget_of(cfg, prefix))
        if no_speech_threshold is not None:
            ns = float(np.exp(LR.detect(model, cfg, mel).log_no_speech_prob))
            w.silent = window_is_silent(ns, w.logprob / (len(w.ids) + 1), no_speech_threshold, logprob_threshold)
        if not w.silent:
            own = min(whole, n // tick)
            w.slices = raw_slices(a.ids, T0, own, whole)
            local, w.advance = SR.seek_rule(a.ids, T0, own, whole)
            base = off // tick
            w.segments = [(base + s, base + e, t) for s, e, t in local]
            segs += w.segments
            ids += sum((t for _, _, t in local), [])
        history, mark = history_after_window(history, mark, w.slices, w.silent, condition, a.temperature, reset_on_temperature)
        w.reset = not w.silent and (not condition or (reset_on_temperature is not None and a.temperature > reset_on_temperature))
        assert not w.reset or mark == len(history)
        wins.append(w)
        off += w.advance * tick
        if off >= len(pcm):
            break
    kept = [w for w in wins if not w.silent] or wins
    return Clip(ids, sum(w.logprob for w in kept) / sum(len(w.ids) + 1 for w in kept), segs, wins, min(w.margin for w in wins), history)
