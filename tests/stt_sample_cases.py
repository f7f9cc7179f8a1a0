"""Fixtures of the temperature-fallback tests (a helper, not a test): the inputs of the sampled-step kernel test, the configurations,
weight sets and clips of the end-to-end test, and the margins both are held by.

Margins.  A sampled pick is decisive when the gap between the two largest perturbed values x / T + g is at least 4 (E / T + G):
E is the project's recorded logit / score error (tests/stt_beam_cases.py) and G the error of the device's winning value on exact
logits - the float32 Gumbel term (two logf) and the rounding of the division and the sum.  A best-of choice, a logprob-threshold
decision and an all-failed choice are decisive at tests/stt_beam_cases.py's MARGIN.  tests/test_stt_fallback_cpu.py asserts every
recorded margin on the CPU, and that the kernel test's rows are decisive but for a share far below the 1 % it may skip.
"""
import dataclasses

import numpy as np

from rho_tts_amd import stt as S
from tests import stt_beam_cases as K
from tests import stt_sample_ref as F
from tests import stt_seek_cases as SC

SR = K.SR
E = K.E
MARGIN = K.MARGIN
# G: the largest |device winning value - float64 winning value| on the same float32 logits.  Measured on an MI355X
# (tests/test_stt_sample_kernel_gpu.py prints it): 4.30e-6 over the six launches of 4096 rows at 300 ids (the worst at T = 0.2, where
# the winning values reach 50 and the division and the sum each round by up to 2^-19 = 1.9e-6; 1.96e-6 at T = 0.6, 1.99e-6 at T = 1) and
# 3.68e-6 at 51865 ids; recorded rounded up.  It holds while |x / T + g| stays below 64, which tests/test_stt_fallback_cpu.py asserts of
# the kernel test's rows.  The score error of one sampled step measured there: 1.19e-6 (E is 3e-5).
G = 6e-6
G_MEASURED = 4.30e-6


def gap_bound(T: float) -> float:
    return 4 * (E / T + G)


# ---------------------------------------------------------------------------------------------- the kernel test
TEMPERATURES = (0.2, 0.6, 1.0)
KERNEL_SEED = 0x5EED0123456789AB
KERNEL_ROWS, KERNEL_STEP, KERNEL_T_INDEX = 4096, 3, 2
SKIP_SHARE_DEVICE, SKIP_SHARE_REFERENCE = 0.01, 0.005


def kernel_config(masked: bool) -> S.SttConfig:
    """The smallest model (vocabulary 300); unmasked: nothing suppressed, at the first step or ever."""
    c = S.tiny_test_config()
    return c if masked else dataclasses.replace(c, suppress_from=0, begin_suppress=())


def kernel_case(T: float, masked: bool, rows: int = KERNEL_ROWS, V: int = 300, seed: int = 11):
    """Random logits (normal, sigma 2) for `rows` rows of one sampled step, with the rows' keys, sample indices and incoming scores.
    The masked case is a first step, so both bits of the suppress mask bind."""
    rng = np.random.default_rng([seed, int(round(T * 10)), int(masked), rows, V])
    return dict(logits=(2.0 * rng.standard_normal((rows, V))).astype(np.float32), key=rng.integers(0, 1 << 20, size=rows).astype(np.int32),
                sample=rng.integers(0, 8, size=rows).astype(np.int32), scores=(-4.0 * rng.random(rows)).astype(np.float32), first_step=bool(masked),
                step=0 if masked else KERNEL_STEP, t_index=KERNEL_T_INDEX, seed=KERNEL_SEED, T=float(T))


def whisper_vocab_config() -> S.SttConfig:
    """A narrow model with Whisper's vocabulary of 51865 ids - no multiple of the 4096 ids a workgroup requests per round trip."""
    return S.SttConfig(d_model=64, heads=2, ffn=128, enc_layers=1, dec_layers=1, n_mels=16, n_ctx=100, chunk_seconds=2, max_new_tokens=8, languages={},
                       no_speech_id=-1)


def whisper_vocab_cases():
    """Two launches of 8 rows at 51865 ids, large logits planted on suppressed ids at the very end of the row (the clamped tail must
    not leak) and on the last id the mask leaves.  With 8 rows none may be skipped: the seed is the first that makes every row decisive."""
    cfg = whisper_vocab_config()
    out = []
    for T, first in ((0.2, False), (1.0, True)):
        case = kernel_case(T, first, rows=8, V=cfg.vocab, seed=12)
        case["logits"][:, -3:] += 6.0
        case["logits"][0, cfg.suppress_from - 1] += 9.0
        out.append(case)
    return out


def reference_rows(case, bad: np.ndarray):
    """The sampled step of every row of `case` at once (tests/stt_sample_ref.py pick_masked, vectorised): picks, their untempered
    log-probabilities, winning values and gaps to the runner-up, in float64.  bad: the ids barred at this step."""
    x = case["logits"].astype(np.float64)
    x[:, bad] = -np.inf
    x[np.isnan(x)] = -np.inf
    rows, V = x.shape
    rh = np.array([F.row_hash(case["seed"], int(k), case["t_index"], int(j), case["step"]) for k, j in zip(case["key"], case["sample"])], dtype=np.uint64)
    g = -np.log(-np.log(F.u_of_k(F.counter_k(rh[:, None], np.arange(V)[None, :]))))
    v = np.where(np.isfinite(x), x / case["T"] + g, -np.inf)
    order = np.argsort(-v, axis=1, kind="stable")           # (stable: the lower id first among equals)
    tok = order[:, 0]
    r = np.arange(rows)
    m = x.max(axis=1)
    lse = m + np.log(np.exp(x - m[:, None]).sum(axis=1))
    return tok, x[r, tok] - lse, v[r, tok], v[r, tok] - v[r, order[:, 1]]


# ---------------------------------------------------------------------------------------------- end to end
# The smallest model: tests/stt_lang_cases.py's (languages, vocabulary 320 grown to 400 with timestamps: tests/stt_seek_cases.py's),
# 2-s windows, 12-token budgets; weight sets A and B of the seek tests.
CFG = SC.seek_test_config()
STATES = SC.STATES
SEED = 789
BEST_OF = 5
TEMPS = (0.0, 0.4, 0.8)
BEAM = 5
# One-window clips (tests/stt_beam_cases.py CLIPS) on weight set A through the fixed-cut call, all three attempts forced: per case the
# smallest margin of an attempt (the beam search's, the best-of choices'), the smallest pick gap of a sampled row, and the margin of the
# all-failed choice, on the CPU reference; tests/test_stt_fallback_cpu.py asserts them.  (Weight set B is too sharp for this: its
# sampled rows repeat one another, and a best-of choice between equal rows has no margin to record.)
EX_CASES = [
    ("A", "clip(1.9, 2)", 3.64e-4, 3.81e-3, 0.646),
    ("A", "zeros 0.7 s", 2.36e-2, 1.04e-2, 0.864),
    ("A", "clip(1.7, 11)", 1.17e-2, 1.81e-2, 0.532),
    ("A", "clip(1.3, 3)", 7.68e-4, 1.45e-3, 0.546),
]
# logprob-triggered fallback on ("A", "clip(1.3, 3)"): its averages are -4.263 (beam), -4.809 (0.4) and -5.069 (0.8)
LOGPROB_CASE = dict(set="A", clip="clip(1.3, 3)", passes=-4.5, fails=-4.0)
# the seek path: one clip of three windows, the ratio script fails the first attempt of the middle window alone; its second attempt
# (temperature 0.4) advances by a whole window where the first advanced by 76 ticks, so the third window starts at tick 176, not 152.
# (weight set, clip, max_initial_timestamp_index, offsets in ticks without fallback, with it)
SEEK_CASE = ("A", "clip(4.1, 5)", 25, [0, 76, 152], [0, 76, 176])
# the seek path under scripts that fail a window's first two attempts (k = 2: the attempt at temperature index 2 stands) and all
# three (k = 3: the attempt with the largest average stands, the ratio taken on text ids with the timestamps stripped): per round of
# the clip - one window each - the number of attempts the script fails; rounds behind the listed ones pass at once.  Every window of
# every case is decisive on the CPU reference at both widths and every attempt has text ids, so the callback is asked for each.
# (clip, fails per round, {beam width: (offsets in ticks, attempts, index of the chosen attempt per window)})
SEEK_SCRIPTS = [
    ("clip(4.1, 5)", [2, 3], {1: ([0, 100, 200], [3, 3, 1], [2, 1, 0]), 5: ([0, 100, 200], [3, 3, 1], [2, 1, 0])}),
    ("clip(4.1, 5)", [3, 2], {1: ([0, 100, 200], [3, 3, 1], [2, 2, 0]), 5: ([0, 76, 176], [3, 3, 1], [0, 2, 0])}),
    ("clip(6.3, 11)", [3, 2], {1: ([0, 100, 200, 300], [3, 3, 1, 1], [0, 2, 0, 0]), 5: ([0, 100, 200, 300], [3, 3, 1, 1], [0, 2, 0, 0])}),
]
SEEK_MAX_INITIAL = 25
# Whisper-tiny dimensions (tests/test_stt_fallback_gpu.py test_whisper_tiny_dimensions): S.SttConfig(max_new_tokens=6), seeded weights
# 789, clip(30.0, SR, 7), beam 1, temperatures (0, 0.4), the first attempt failed by the script.  On the CPU reference: the beam
# attempt's margin, the sampled attempt's best-of margin and its smallest pick gap.
TINY_CASE = dict(max_new_tokens=6, clip=(30.0, 7), temperatures=(0.0, 0.4), margin_beam=0.239, margin_best_of=0.0933, gap=0.0581)


def tiny_reference():
    """The restated loop on the Whisper-tiny case -> (configuration, seeded state, clip, Fallback)."""
    from oracle import whisper as OW
    from tests import stt_beam_ref as R
    from tests.test_oracle_whisper import clip
    o = TINY_CASE
    cfg = S.SttConfig(max_new_tokens=o["max_new_tokens"])
    state = S.synthetic_state(cfg, 789)
    x = clip(o["clip"][0], SR, o["clip"][1])
    ret = iter([9.0, 1.0])
    fb = F.window_fallback(OW.build(cfg, state), cfg, R.window_mels(cfg, x, SR)[0], 1, BEST_OF, o["temperatures"], SEED, 0, ratio=lambda ids: next(ret),
                           logprob_threshold=None)
    return cfg, state, x, fb
