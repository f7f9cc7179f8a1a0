"""Reference of language detection and the no-speech probability (rt_stt_detect_language, rt_stt_transcribe_ex) in float64: a helper
of the language tests, not a test.

The rule ("language and no-speech").  For one window let z be the decoder's logits over the whole vocabulary
after a one-token pass on start-of-transcript alone - position 0, over the window's encoder states, nothing suppressed.
  language        the configured id with the largest z; the lowest id on ties, a NaN never
                  (transformers generation_whisper.py detect_language: every other id to -inf, argmax)
  language prob.  softmax of z restricted to the configured ids, at that id
  no-speech prob. softmax of z over the whole vocabulary at the no-speech id
                  (transformers logits_process.py WhisperNoSpeechDetection: softmax of the start-of-transcript logits)
NaNs take no part in either sum.  ``probe`` is the rule on given logits (what k_stt_probe computes); ``window_logits`` runs
transformers' Whisper as oracle/whisper.py builds it; ``detect`` is the two together with the language margin.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Sequence

import numpy as np
import torch

INF = float("inf")


@dataclass
class Probe:
    language: int            # token id
    log_language_prob: float
    log_no_speech_prob: float
    margin: float            # top-1 minus top-2 language logit (inf with one candidate)


def _lse(x: np.ndarray) -> float:
    x = x[~np.isnan(x)]
    m = x.max() if x.size else -INF
    return float(m + np.log(np.exp(x - m).sum())) if np.isfinite(m) else -INF


def probe(z, lang_ids: Sequence[int], no_speech_id: int) -> Probe:
    z = np.asarray(z, dtype=np.float64)
    ids = sorted(int(i) for i in lang_ids)                       # ascending: the first maximum is the lowest id
    zl = z[ids]
    ok = ~np.isnan(zl)
    if not ok.any():
        return Probe(ids[0], -INF, float(z[no_speech_id] - _lse(z)) if not np.isnan(z[no_speech_id]) else -INF, 0.0)
    masked = np.where(ok, zl, -INF)
    k = int(np.argmax(masked))
    rest = np.delete(masked, k)
    lp = float(masked[k] - _lse(zl)) if np.isfinite(masked[k]) else -INF
    ns = float(z[no_speech_id] - _lse(z)) if not np.isnan(z[no_speech_id]) and np.isfinite(_lse(z)) else -INF
    return Probe(ids[k], lp, ns, float(masked[k] - rest.max()) if rest.size and np.isfinite(masked[k]) else INF)


@torch.no_grad()
def window_logits(model, cfg, mel: torch.Tensor) -> np.ndarray:
    """z of one window: the model's forward with decoder_input_ids = [[start-of-transcript]] (float32, returned as float64)."""
    enc = model.model.encoder(mel[None])
    return model(encoder_outputs=enc, decoder_input_ids=torch.tensor([[int(cfg.prefix[0])]])).logits[0, -1].double().numpy()


def detect(model, cfg, mel: torch.Tensor) -> Probe:
    return probe(window_logits(model, cfg, mel), list(cfg.languages.values()), cfg.no_speech_id)


def hf_detect_language(model, cfg, mel: torch.Tensor) -> int:
    """transformers' own ``detect_language`` on the window's encoder states, with the configured ids as ``lang_to_id``."""
    import copy
    from transformers.modeling_outputs import BaseModelOutput
    gc = copy.deepcopy(model.generation_config)
    gc.lang_to_id = {f"<|{k}|>": int(v) for k, v in cfg.languages.items()}
    gc.decoder_start_token_id = int(cfg.prefix[0])
    with torch.no_grad():
        enc = model.model.encoder(mel[None])
    return int(model.detect_language(encoder_outputs=BaseModelOutput(last_hidden_state=enc.last_hidden_state), generation_config=gc)[0])


def first_window_mels(cfg, clips: List[np.ndarray], sr: int) -> List[torch.Tensor]:
    from tests import stt_beam_ref as R
    return [R.window_mels(cfg, x, sr)[0] for x in clips]
