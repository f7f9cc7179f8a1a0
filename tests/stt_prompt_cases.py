"""Fixtures of the prompt tests (a helper, not a test): the configuration, the weight sets and the cases whose ids, segments, offsets,
prompt lengths and reset flags are held against the float64 reference (tests/stt_prompt_ref.py).

The configuration is ``seek_test_config()`` (tests/stt_seek_cases.py: vocabulary 400, n_text_ctx 32 - a prompt of at most 15 ids and a
prefix of at most 19 tokens) with <|startofprev|> = 295.  Every special id of that vocabulary is taken - 290 end-of-sequence, 291
start-of-transcript, 292 .. 295 the languages of tests/stt_lang_cases.py LANGUAGES, 296 transcribe, 297 no-speech, 298 no-timestamps,
299 .. 399 timestamps; 294 is "ja" there - so the configuration here leaves "ko" out of its languages, which frees 295.  No case
detects a language, so nothing else changes: without a policy a case decodes what tests/stt_seek_cases.py records.

Cases are the 16 (case, width) pairs of tests/stt_seek_cases.py, each run conditioned on previous text, and conditioned with the
4-id initial prompt INITIAL.  A pair is kept when BOTH runs have a margin of at least MARGIN = 4 E on the CPU reference; three pairs
are left out for a run below it (set A at width 5: clip(5.0, 2) limited, 7.83e-5; clip(6.3, 11), 1.15e-4; clip(4.1, 5), 5.21e-5, all
three in the run with the initial prompt).  tests/test_stt_prompt_cpu.py asserts every recorded figure and the conditions the cases
meet together.
"""
import dataclasses

from rho_tts_amd import stt as S
from tests import stt_seek_cases as SC

SR = SC.SR
E = SC.E
MARGIN = SC.MARGIN
# Measured on an MI355X (tests/test_stt_prompt_gpu.py and tests/test_stt_prompt_kernel_gpu.py print them): the largest
# |device - reference| of a window's cumulative log-probability over the cases below, and of the log-softmax behind the ragged
# prefix pass on the small model and behind the 227-token prefix at Whisper-tiny dimensions.  The bound is 4 E = 1.2e-4.
# (the loop's worst: set B, clip(7.0, 3), width 5, conditioned; the budget cases 2.98e-5, the fallback interplay 1.16e-5)
# ("logits": the raw last-row logits of the prefix pass, which carry the same bound as their log-softmax)
MEASURED = {"tiny": 3.92e-5, "tiny prefix pass": 6.78e-5, "tiny prefix pass logits": 5.34e-5, "whisper-tiny prefix pass": 1.96e-5,
            "whisper-tiny prefix pass logits": 1.95e-5, "whisper-tiny three steps": 1.98e-5}

SOT_PREV = 295
INITIAL = [11, 57, 123, 204]


def prompt_test_config() -> S.SttConfig:
    c = SC.seek_test_config()
    return dataclasses.replace(c, languages={k: v for k, v in c.languages.items() if v != SOT_PREV}, sot_prev_id=SOT_PREV)


STATES = SC.STATES
CLIPS = SC.CLIPS

# (weight set, clip, max_initial_timestamp_index, beam width, {run: (rounds, margin on the CPU reference)})
CASES = [
    ("A", "clip(5.0, 2)", -1, 1, {"conditioned": (3, 2.57e-2), "initial": (3, 4.65e-2)}),     # conditioned: one-id windows add nothing, no prompt ever
    ("A", "clip(5.0, 2)", -1, 5, {"conditioned": (3, 9.88e-4), "initial": (4, 5.72e-3)}),     # every window consumed whole (d); initial: the cap is reached (b)
    ("A", "clip(5.0, 2)", 25, 1, {"conditioned": (4, 2.33e-2), "initial": (3, 2.08e-2)}),     # the third window discards a tail of two ids (c)
    ("A", "clip(6.3, 11)", 25, 1, {"conditioned": (4, 1.26e-3), "initial": (4, 4.18e-3)}),
    ("A", "clip(4.1, 5)", 25, 1, {"conditioned": (3, 1.13e-2), "initial": (3, 1.63e-2)}),
    ("B", "clip(5.0, 2)", 25, 1, {"conditioned": (3, 4.81e-2), "initial": (3, 7.1e-2)}),      # prompts of 7 and 11 ids (a), tails of 5 and 8 (c)
    ("B", "clip(5.0, 2)", 25, 5, {"conditioned": (4, 4.51e-3), "initial": (4, 6.11e-3)}),
    ("B", "clip(6.3, 11)", -1, 1, {"conditioned": (5, 1.24e-1), "initial": (5, 1.26e-1)}),
    ("B", "clip(6.3, 11)", -1, 5, {"conditioned": (5, 9.03e-3), "initial": (5, 6.39e-4)}),
    ("B", "clip(7.0, 3)", 25, 1, {"conditioned": (4, 5.03e-3), "initial": (4, 1.54e-2)}),
    ("B", "clip(7.0, 3)", 25, 5, {"conditioned": (5, 4.01e-4), "initial": (5, 4.86e-3)}),
    ("B", "clip(4.1, 5)", -1, 1, {"conditioned": (3, 1.96e-2), "initial": (3, 1.36e-2)}),
    ("B", "clip(4.1, 5)", -1, 5, {"conditioned": (3, 2.03e-2), "initial": (4, 4.21e-3)}),
]
LEFT_OUT = [("A", "clip(5.0, 2)", 25, 5), ("A", "clip(6.3, 11)", 25, 5), ("A", "clip(4.1, 5)", 25, 5)]

# The binding per-window budget (g): dataclasses.replace(cfg, max_new_tokens=16), conditioned.  A window behind a full prompt has a
# prefix of 19 tokens and 32 - 19 = 13 steps, one without a prompt 16: one clip's windows hit both.
# (weight set, clip, max_initial_timestamp_index, beam width, rounds, margin, the windows' budgets, the ids they decoded)
BUDGET_CASES = [
    ("A", "clip(5.0, 2)", 25, 1, 4, 2.33e-2, [16, 16, 16, 13], [4, 4, 16, 13]),
    ("A", "clip(5.0, 2)", 25, 5, 4, 2.84e-4, [16, 16, 16, 13], [4, 4, 16, 4]),
    ("B", "clip(6.3, 11)", -1, 1, 5, 1.24e-1, [16, 16, 16, 13, 13], [16, 16, 16, 13, 13]),
    ("B", "clip(6.3, 11)", -1, 5, 5, 6.83e-3, [16, 13, 13, 13, 13], [16, 13, 13, 13, 13]),
]


def budget_config() -> S.SttConfig:
    return dataclasses.replace(prompt_test_config(), max_new_tokens=16)


# The fallback interplay: weight set A, clip(6.3, 11), max_initial_timestamp_index 25, temperatures (0, 0.2, 0.4, 0.6), best_of 5, seed
# 789, no logprob threshold; the ratio script fails no attempt of the first window, one of the second and three of the third.  On the
# CPU reference at both widths: the chosen temperatures, the prompt lengths (the fourth window starts from an empty prompt: 0.6 is
# above the reset temperature, 0.2 is not) and the reset flags; every window is decisive (stt_sample_ref.decisive).
FALLBACK_CASE = dict(set="A", clip="clip(6.3, 11)", max_initial=25, temperatures=(0.0, 0.2, 0.4, 0.6), best_of=5, seed=789, fails=[0, 1, 3],
                     chosen=[0.0, 0.2, 0.6, 0.0], attempts=[1, 2, 4, 1], prompts=[0, 12, 15, 0], reset=[False, False, True, False])

# Whisper-tiny dimensions (tests/test_stt_prompt_kernel_gpu.py): S.SttConfig(max_new_tokens=3, timestamp_begin=50364), seeded weights
# 789, clip(4.0, SR, 3), an initial prompt of 223 seeded ids (a prefix of 227 tokens), width 1: the margin of the three greedy steps
# on the CPU reference
TINY_CASE = dict(margin=1.79e-3)


def run_kwargs(run: str) -> dict:
    """What a run of a case passes to ``NativeSTT.set_prompt`` (and, as ``initial``, to the reference)."""
    return {"conditioned": dict(initial_ids=None), "initial": dict(initial_ids=list(INITIAL))}[run]
