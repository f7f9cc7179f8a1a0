"""Reference of the speech-to-text beam search (rt_stt_transcribe_beam) in float64: a helper of the beam tests, not a test.

The rule (Whisper's published BeamSearchDecoder with faster-whisper's defaults - patience 1, length penalty 1).
Per window and beam width B: up to B live beams in order, each with the tokens behind the forced prefix and a cumulative score, and a
finished list F of at most B entries in admission order; step 0 starts from ONE empty beam of score 0.  Per step every live beam j
offers its B + 1 largest log-probabilities (log-softmax over the whole vocabulary of the logits masked as for the greedy rule; lower
id on ties) as candidates of score s_j + lp.  The window's candidates are sorted by score, descending (ties: lower beam, then lower
id) and walked: an end-of-sequence candidate is newly finished, any other becomes the next live beam, until B next beams are taken.
Newly finished entries join F in walk order while it has room.  The window is complete when F is full or after
min(max_new_tokens, n_text_ctx - n_prefix) steps; live beams fill F up at the end, in order.  The result is the entry with the
largest score / (n_tokens + 1), the earlier one on a tie.

``beam_step`` is one step on given logits (what k_stt_beam_select computes), ``beam_search`` the whole rule on transformers' Whisper
(oracle/whisper.py builds it), with the case's decisive margin; ``rescore`` is the teacher-forced score of given ids.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List, Optional, Tuple

import numpy as np
import torch

INF = float("inf")


def masks(cfg) -> Tuple[np.ndarray, np.ndarray]:
    """(never, not-as-the-first-token) boolean masks over the vocabulary: the greedy rule's (oracle/whisper.py greedy)."""
    never = np.zeros(cfg.vocab, dtype=bool)
    if cfg.suppress_from > 0:
        never[cfg.suppress_from:] = True
        never[cfg.eos_id] = False
    for t in getattr(cfg, "suppress_tokens", ()):
        if 0 <= int(t) < cfg.vocab and int(t) != cfg.eos_id:
            never[int(t)] = True
    begin = np.zeros(cfg.vocab, dtype=bool)
    for t in cfg.begin_suppress:
        begin[int(t)] = True
    return never, begin


def log_softmax(logits: np.ndarray, bad: np.ndarray) -> np.ndarray:
    """float64 log-softmax of one row over the allowed ids; masked ids and NaNs are -inf."""
    x = np.asarray(logits, dtype=np.float64).copy()
    x[bad | np.isnan(x)] = -INF
    m = x.max()
    if not np.isfinite(m):
        return np.full_like(x, -INF)
    return x - (m + np.log(np.exp(x - m).sum()))


@dataclass
class Step:
    next: List[Tuple[int, int, float]]          # (token, parent beam, score) of the next live beams, in order
    finished: List[Tuple[int, float]]           # (parent beam, score) of the entries this step admitted to F, in order
    n_fin: int                                  # |F| after the step
    done: bool                                  # F is full (or no beam is left)
    walk_gap: float                             # last candidate the walk consumed - first it left out (inf: none left out)
    order_gaps: List[float] = field(default_factory=list)   # gaps between consecutive consumed candidates, and the boundary's


def beam_step(logits, scores, B: int, eos: int, never: np.ndarray, begin: Optional[np.ndarray] = None, first_step: bool = False, n_fin: int = 0) -> Step:
    """One step for one window: logits [n_live][V], scores [n_live] (the live beams, in order)."""
    logits = np.asarray(logits)
    n_live, V = logits.shape
    bad = never | begin if (first_step and begin is not None) else never
    lp = np.stack([log_softmax(logits[j], bad) for j in range(n_live)]) if n_live else np.zeros((0, V))
    sc = np.asarray(scores, dtype=np.float64)[:, None] + lp
    cands = []                                  # the rule, literally: B + 1 per beam ...
    for j in range(n_live):
        order = np.lexsort((np.arange(V), -lp[j]))[:B + 1]
        cands += [(float(sc[j, t]), j, int(t)) for t in order if lp[j, t] > -INF]
    cands.sort(key=lambda c: (-c[0], c[1], c[2]))            # ... sorted by score, then beam, then id
    nxt, newly, consumed = [], [], 0
    for s, j, t in cands:
        if len(nxt) >= B:
            break
        consumed += 1
        if t == eos:
            newly.append((j, s))
        else:
            nxt.append((t, j, s))
    admitted = newly[:max(0, B - n_fin)]
    # the same walk over ALL candidates of the window (no B + 1 cut) consumes the same prefix; what follows it is the first left out
    flat = sc.reshape(-1)
    beams, toks = np.divmod(np.arange(flat.size), V)
    full = np.lexsort((toks, beams, -flat))
    full = full[flat[full] > -INF]
    assert [(int(beams[i]), int(toks[i])) for i in full[:consumed]] == [(j, t) for _, j, t in cands[:consumed]]
    line = [float(flat[i]) for i in full[:consumed + 1]]
    gaps = [a - b for a, b in zip(line[:-1], line[1:])]
    walk_gap = gaps[consumed - 1] if len(line) > consumed and consumed else INF
    n_fin += len(admitted)
    return Step(nxt, admitted, n_fin, n_fin >= B or not nxt, walk_gap, gaps)


@dataclass
class Result:
    ids: List[int]
    score: float                                # cumulative log-probability of the chosen entry (end-of-sequence included if it ended)
    norm: float                                 # score / (len(ids) + 1): what the call reports
    ended: bool                                 # the chosen entry ended on end-of-sequence (before the budget)
    margin: float                               # the decisive margin (see search)
    final_margin: float                         # best - second-best normalised score
    entries: List[Tuple[List[int], float, bool]] = field(default_factory=list)    # F at the end: (ids, score, ended)


def budget_of(cfg, max_new: Optional[int] = None) -> int:
    return min(int(max_new or cfg.max_new_tokens), cfg.n_text_ctx - len(cfg.prefix))


@torch.no_grad()
def _logits(model, enc, cfg, beams: List[List[int]]) -> np.ndarray:
    """Logits behind prefix + tokens of every beam: [len(beams)][vocab] float64 (the model runs in float32)."""
    from transformers.modeling_outputs import BaseModelOutput
    ids = torch.tensor([[int(t) for t in cfg.prefix] + b for b in beams])
    eo = BaseModelOutput(last_hidden_state=enc.expand(len(beams), -1, -1))
    return model(encoder_outputs=eo, decoder_input_ids=ids).logits[:, -1].double().numpy()


@torch.no_grad()
def encode(model, mel: torch.Tensor) -> torch.Tensor:
    return model.model.encoder(mel[None]).last_hidden_state


def search(step_logits, B: int, budget: int, eos: int, never: np.ndarray, begin: Optional[np.ndarray] = None) -> Result:
    """The rule over any model: step_logits(beams) -> logits [len(beams)][V] behind the forced prefix + each beam's tokens.
    The decisive margin is the smallest of: the gap between the last candidate a step's walk consumed and the first it left out,
    over all steps; the gaps between consecutive newly finished entries that were admitted; the gaps between the live beams that
    fill F up at the end and the first that does not; the gap between the best and the second-best normalised final score.  A
    device whose scores are off by less than half of it decides everything alike."""
    beams: List[List[int]] = [[]]
    scores = [0.0]
    F: List[Tuple[List[int], float, bool]] = []
    margin = INF
    for step in range(budget):
        st = beam_step(step_logits(beams), scores, B, eos, never, begin, step == 0, len(F))
        margin = min(margin, st.walk_gap)
        fin = [s for _, s in st.finished]
        margin = min([margin] + [a - b for a, b in zip(fin[:-1], fin[1:])])
        F += [(list(beams[j]), s, True) for j, s in st.finished]
        beams, scores = [beams[j] + [t] for t, j, _ in st.next], [s for _, _, s in st.next]
        if st.done:
            break
    if len(F) < B:
        room = B - len(F)
        margin = min([margin] + [a - b for a, b in zip(scores[:room], scores[1:room + 1])])
        F += [(b, s, False) for b, s in zip(beams[:room], scores[:room])]
    norms = [s / (len(i) + 1) for i, s, _ in F]
    best = int(np.argmax(norms))                               # (the first maximal entry)
    final = min([norms[best] - n for k, n in enumerate(norms) if k != best] or [INF])
    ids, score, ended = F[best]
    return Result(list(ids), score, norms[best], ended, min(margin, final), final, F)


@torch.no_grad()
def beam_search(model, cfg, mel: torch.Tensor, B: int, max_new: Optional[int] = None) -> Result:
    """The rule on one window's log-mel features, on transformers' Whisper as oracle/whisper.py builds it."""
    enc = encode(model, mel)
    never, begin = masks(cfg)
    return search(lambda beams: _logits(model, enc, cfg, beams), B, budget_of(cfg, max_new), cfg.eos_id, never, begin)


@torch.no_grad()
def rescore(model, cfg, mel: torch.Tensor, ids: List[int], ended: bool, max_new: Optional[int] = None) -> float:
    """Teacher-forced cumulative log-probability (float64 log-softmax of the masked logits) of `ids` behind the forced prefix, and of
    end-of-sequence behind them if the hypothesis ended."""
    enc = encode(model, mel)
    never, begin = masks(cfg)
    seq = list(ids) + ([cfg.eos_id] if ended else [])
    total = 0.0
    for k, t in enumerate(seq):
        lg = _logits(model, enc, cfg, [list(ids[:k])])[0]
        total += float(log_softmax(lg, never | begin if k == 0 else never)[t])
    return total


def window_mels(cfg, pcm: np.ndarray, sr: int) -> List[torch.Tensor]:
    """The log-mel features of every chunk_seconds window of a clip, cut as the native call cuts it."""
    from oracle import whisper as OW
    pcm = np.asarray(pcm, dtype=np.float32)
    win = int(cfg.chunk_seconds) * int(sr)
    out = []
    for w in range(max(1, -(-len(pcm) // win))):
        x = pcm[w * win:(w + 1) * win]
        out.append(OW.log_mel(cfg, OW.resample(x, sr, cfg.sample_rate) if sr != cfg.sample_rate else x))
    return out


def clip_search(model, cfg, pcm: np.ndarray, sr: int, B: int) -> Tuple[List[int], float, List[Result]]:
    """A clip of any length: its windows' ids joined, sum of the windows' scores / sum of (ids + 1), and the windows' results."""
    res = [beam_search(model, cfg, m, B) for m in window_mels(cfg, pcm, sr)]
    return sum((r.ids for r in res), []), sum(r.score for r in res) / sum(len(r.ids) + 1 for r in res), res
