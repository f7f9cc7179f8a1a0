"""Fixtures of the seek tests (a helper, not a test): the smallest model with timestamp ids, two weight sets, the clips and the cases
whose ids, segments and offsets are held against the float64 reference (tests/stt_seek_ref.py).

The configuration is ``lang_test_config()`` (tests/stt_lang_cases.py) grown to hold timestamps: vocabulary 400, <|notimestamps|> 298,
timestamp ids 299 .. 399 (101 of them: the 2-s window in ticks of 0.02 s), prefix (291, 292, 296, 298).

Weight sets are A and B of the beam tests (tests/stt_beam_cases.py) with the timestamp rows of the tied embedding scaled - x 2 in A,
x 3 in B - so that A ends its windows early, on closed pairs or a single trailing timestamp, and B runs to the budget and leaves
tails behind its last pair.

The conditions the cases meet together, on the CPU reference (tests/test_stt_seek_cpu.py asserts them and every margin, so that a
change of the reference's arithmetic fails there and does not flake on the GPU):
  (a) a window closes a pair and discards a non-empty tail, with an advance below a whole window;
  (b) a window ends on a single trailing timestamp;
  (c) a window has no pair at all;
  (d) the logsumexp rule decides both ways;
  (e) max_initial_timestamp_index binds in one case (the unlimited case of the same clip starts later) and is -1 in another.
A case's margin is the smallest, over its windows, of: every step's walk gap and beam boundary and the final choice
(stt_beam_ref.search) and every row's |lse(timestamps) - max(text)|.
"""
import dataclasses

import numpy as np
import torch

from rho_tts_amd import stt as S
from tests import stt_beam_cases as K
from tests import stt_lang_cases as L
from tests.test_oracle_whisper import clip

SR = K.SR
# Measured on an MI355X (tests/test_stt_seek_gpu.py prints them): the largest |device - reference| of a window's cumulative
# log-probability over the cases below, and over the two clips at Whisper-tiny dimensions.  The bound is 4 E = 1.2e-4.
E = K.E
MARGIN = K.MARGIN
# (a window here is up to 12 tokens, timestamps among them, and its error is that of their sum: 3.98e-5 on set B, clip(7.0, 3), width 1)
MEASURED = {"tiny": 3.98e-5, "whisper-tiny": 2.04e-5}

VOCAB, TIMESTAMP_BEGIN = 400, 299


def seek_test_config() -> S.SttConfig:
    return dataclasses.replace(L.lang_test_config(), vocab=VOCAB, timestamp_begin=TIMESTAMP_BEGIN)


def _scaled(base, cfg, ts_scale):
    state = base(cfg)
    w = state["model.decoder.embed_tokens.weight"].clone().float()
    w[cfg.timestamp_begin:] *= ts_scale
    state["model.decoder.embed_tokens.weight"] = w.to(torch.bfloat16)
    return state


def state_a(cfg):
    return _scaled(K.state_a, cfg, 2.0)


def state_b(cfg):
    return _scaled(K.state_b, cfg, 3.0)


STATES = {"A": state_a, "B": state_b}

CLIPS = {
    "clip(5.0, 2)": lambda: clip(5.0, SR, 2),
    "clip(6.3, 11)": lambda: clip(6.3, SR, 11),
    "clip(4.1, 5)": lambda: clip(4.1, SR, 5),
    "clip(7.0, 3)": lambda: clip(7.0, SR, 3),
}

# (weight set, clip, max_initial_timestamp_index, {beam width: (rounds, margin on the CPU reference)})
CASES = [
    ("A", "clip(5.0, 2)", -1, {1: (3, 2.57e-2), 5: (3, 2.92e-4)}),       # width 1: no pair in any window (c); the unlimited twin of the next
    ("A", "clip(5.0, 2)", 25, {1: (5, 1.05e-2), 5: (4, 2.84e-4)}),       # the limit binds (e): <|0.08|> where the twin starts at <|1.52|>
    ("A", "clip(6.3, 11)", 25, {1: (4, 1.33e-2), 5: (4, 3.83e-4)}),      # three windows end on a single trailing timestamp (b)
    ("A", "clip(4.1, 5)", 25, {1: (3, 9.53e-3), 5: (3, 2.87e-4)}),
    ("B", "clip(5.0, 2)", 25, {1: (3, 2.08e-2), 5: (4, 2.1e-3)}),        # a pair, a tail of five ids discarded, advance 96 (a)
    ("B", "clip(6.3, 11)", -1, {1: (4, 1.24e-1), 5: (4, 1.03e-3)}),      # (a) again: advance 77
    ("B", "clip(7.0, 3)", 25, {1: (5, 1.63e-2), 5: (6, 2.22e-3)}),
    ("B", "clip(4.1, 5)", -1, {1: (3, 1.96e-2), 5: (3, 8.44e-3)}),
]
# the case of kind (a) the re-decoding test uses: its first window closes its last pair at tick 96 and discards five ids behind it
REDECODED = ("B", "clip(5.0, 2)", 25)

# The silence rule's clip: 2 s of speech - a window that ends on a single trailing timestamp, so it is consumed whole - and 4 s of
# zeros, on weight set A with max_initial_timestamp_index 25.  Seeded weights give no meaningful no-speech probability (every window's
# is about 0.002), so the thresholds separate the windows by their average log-probability: -2.40 for the speech window, -2.53 for a
# window of zeros.
SILENCE = {"set": "A", "max_initial": 25, "no_speech_threshold": 0.001, "logprob_threshold": -2.46}


def speech_then_silence():
    return np.concatenate([clip(2.0, SR, 11), np.zeros(4 * SR, dtype=np.float32)])
