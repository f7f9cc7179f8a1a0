"""Fixtures of the beam-search tests (a helper, not a test): the smallest model with two sets of seeded weights, the clips, and the
cases whose ids are held against the float64 oracle (tests/stt_beam_ref.py) - chosen by decisive margin, not by hand.

E, the largest |device cumulative score - rescore of the same ids| measured on an MI355X over every candidate below, and MARGIN, the
smallest decisive margin a case must have to be held to the oracle's ids (>= 4 E: both hypotheses at a boundary drifting in opposite
directions, times two), are recorded here; tests/test_stt_beam_cpu.py asserts every case's margin on the CPU, so that a change of
the oracle's arithmetic that erodes a margin fails there and does not flake on the GPU.
"""
import numpy as np
import torch

from rho_tts_amd import stt as S
from tests.test_oracle_whisper import clip

SR = 24000
# Measured on an MI355X: 1.85e-5 over the 18 cases below (the worst: set A, clip(1.3, 3), width 2)
# and 2.95e-5 on the three clips at Whisper-tiny dimensions (tests/test_stt_beam_gpu.py); recorded rounded up.
E = 3e-5
MARGIN = 4 * E                # 1.2e-4: the smallest margin below is 40 times that

CLIPS = {
    "clip(1.9, 2)": lambda: clip(1.9, SR, 2),
    "zeros 0.7 s": lambda: np.zeros(int(0.7 * SR), dtype=np.float32),
    "clip(1.7, 11)": lambda: clip(1.7, SR, 11),
    "clip(2.0, 5)": lambda: clip(2.0, SR, 5),
    "clip(1.3, 3)": lambda: clip(1.3, SR, 3),
}


def state_a(cfg):
    """Weight set A: the end-of-sequence row of the tied embedding / LM head x 6.0, bf16-rounded (tests/test_stt_batch_gpu.py's
    early_ending_state): hypotheses end at different steps."""
    state = S.synthetic_state(cfg, 789)
    w = state["model.decoder.embed_tokens.weight"].clone()
    w[cfg.eos_id] = (w[cfg.eos_id].float() * 6.0).to(torch.bfloat16).to(w.dtype)
    state["model.decoder.embed_tokens.weight"] = w
    return state


def state_b(cfg):
    """Weight set B: every row of the tied embedding x 4, the end-of-sequence row x 1.5 of its seeded value instead, bf16-rounded:
    sharper logits, no early end."""
    state = S.synthetic_state(cfg, 789)
    w = state["model.decoder.embed_tokens.weight"].clone().float() * 4.0
    w[cfg.eos_id] = w[cfg.eos_id] / 4.0 * 1.5
    state["model.decoder.embed_tokens.weight"] = w.to(torch.bfloat16)
    return state


STATES = {"A": state_a, "B": state_b}

# (weight set, clip, beam width, decisive margin on the CPU oracle, ids, ends on end-of-sequence, differs from greedy)
CASES = [
    ("A", "clip(1.9, 2)", 3, 3.2e-2, 1, True, True),
    ("A", "clip(1.9, 2)", 5, 1.29e-2, 1, True, True),
    ("A", "zeros 0.7 s", 2, 1.26e-2, 5, True, True),
    ("A", "clip(1.7, 11)", 2, 1.8e-2, 2, True, True),
    ("A", "clip(1.7, 11)", 3, 2.7e-2, 3, True, True),
    ("A", "clip(1.7, 11)", 5, 4.99e-3, 4, True, True),
    ("A", "clip(2.0, 5)", 2, 8.12e-3, 1, True, True),
    ("A", "clip(2.0, 5)", 3, 8.27e-3, 3, True, True),
    ("A", "clip(1.3, 3)", 2, 6.63e-3, 4, True, True),
    ("A", "clip(1.3, 3)", 5, 5.14e-3, 3, True, True),
    ("B", "clip(1.9, 2)", 2, 6.61e-2, 12, False, False),
    ("B", "clip(1.7, 11)", 2, 1.98e-1, 12, False, True),
    ("B", "clip(1.7, 11)", 3, 9.79e-2, 12, False, True),
    ("B", "clip(1.7, 11)", 5, 9.79e-2, 12, False, True),
    ("B", "clip(2.0, 5)", 2, 5.96e-2, 12, False, True),
    ("B", "clip(2.0, 5)", 5, 3.24e-2, 12, False, True),
    ("B", "clip(1.3, 3)", 3, 1.72e-2, 12, False, True),
    ("B", "clip(1.3, 3)", 5, 1.32e-2, 12, False, True),
]
