"""k_stt_beam_select and k_stt_sample_select state the decoding step rule through the same device functions (stt_step_ids,
stt_row_norm, stt_ts_next in csrc/stt.hip): this file pins that the two kernels normalise a row identically.  The same logits row
and the same incoming score go through rt_debug_stt_beam_step[_ts] and rt_debug_stt_sample_step[_ts]; the sampled pick is the beam's
first candidate of that row, so both write s + (x[id] - lse) from the same lse: the outgoing scores are equal BIT FOR BIT, and under
the timestamp rule so is the row's outgoing history state.

The pick is made the beam's first candidate by the temperature: the Gumbel term g = -log(-log(u)), u in [2^-24, 1 - 2^-24], lies in
[-2.82, 16.64], so two ids whose logits are 20 T apart cannot change places.  Every row is planted so that the largest logit among
the ids the rule leaves leads the runner-up by at least that (LEAD, asserted on the CPU with tests/stt_sample_ref.py before the
device is asked); seeds are pinned and no row is skipped."""
import ctypes as C

import numpy as np
import pytest

from rho_tts_amd import _native
from tests import stt_beam_ref as R
from tests import stt_sample_cases as FC
from tests import stt_sample_ref as F
from tests import stt_seek_cases as SC
from tests import stt_seek_ref as SR
from tests import test_stt_beam_kernel_gpu as KB
from tests import test_stt_sample_kernel_gpu as KS
from tests import test_stt_seek_kernel_gpu as KT

pytestmark = pytest.mark.gpu

T = 0.05
LEAD = 20.0 * T
SEED, T_INDEX = FC.KERNEL_SEED, FC.KERNEL_T_INDEX
T0 = SC.TIMESTAMP_BEGIN
OFFSETS = (-6.0, 0.0, 7.0)          # on the timestamp ids, as tests/test_stt_sample_kernel_gpu.py: the logsumexp rule decides both ways


@pytest.fixture(scope="module")
def ctx():
    c = _native.Context(0)
    yield c
    c.close()


def model(ctx, cfg):
    m = KS.model(ctx, cfg)
    KB.declare(m.lib)
    i32p, f32p = C.POINTER(C.c_int32), C.POINTER(C.c_float)
    m.lib.rt_debug_stt_beam_step_ts.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, f32p, C.c_int32, C.c_int32, i32p, i32p, i32p, C.c_int32, C.c_int32,
                                                C.c_int32, i32p, i32p, i32p, i32p, f32p, i32p, i32p, f32p, i32p, i32p, i32p, i32p, i32p]
    return m


def bits(a):
    return np.asarray(a, dtype=np.float32).view(np.uint32)


def leaders(rows, picks):
    """rows: the float64 logits of every row with the barred ids at -inf; picks: the reference's sampled picks.  The largest id of
    each row, after asserting that it leads by LEAD and that the reference picks it."""
    top = []
    for r, (x, p) in enumerate(zip(rows, picks)):
        order = np.argsort(-x, kind="stable")
        assert x[order[0]] - x[order[1]] >= LEAD, (r, x[order[0]], x[order[1]])
        assert p.tok == order[0], (r, p.tok, order[0])
        top.append(int(order[0]))
    return top


def first_candidate(got, w, B, tok, eos):
    """The beam step's entry for candidate `tok` of window w's row 0 (every case here has one live row per window): the finished
    list's when it is end-of-sequence, else the first next beam's -> (score, output row or None)."""
    if tok == eos:
        assert got["n_fin"][w] == 1 and got["fin_beam"][w * B] == 0, (w, got["n_fin"][w])
        return got["fin_score"][w * B], None
    assert got["tok"][w * B] == tok and got["par"][w * B] == w * B, (w, got["tok"][w * B], tok)
    return got["score"][w * B], w * B


def test_every_history_shape_at_every_offset(ctx):
    """21 rows, vocabulary 400: the seven history shapes at the three offsets; a text leader and a timestamp leader per row, and
    end-of-sequence as the text leader where a pair is being closed (the beam step then files it in the finished list)."""
    cfg = SC.seek_test_config()
    eos, V = cfg.eos_id, cfg.vocab
    never, begin = SR.suppress_mask(cfg)
    hists = [KS.SHAPES[r % 7] for r in range(21)]
    rng = np.random.default_rng(2301)
    lg = rng.uniform(-8.0, 2.0, size=(21, V)).astype(np.float32)
    free_text = np.flatnonzero(~never[:eos])
    for r in range(21):
        lg[r, T0:] += OFFSETS[r // 7]
        lg[r, eos if r % 7 == 4 else rng.choice(free_text)] += 12.0
        lg[r, rng.integers(T0 + 51, V)] += 12.0                               # (above every shape's last timestamp)
    scores = (-4.0 * rng.random(21)).astype(np.float32)
    key, sample = rng.integers(0, 1 << 20, size=21), rng.integers(0, 8, size=21)
    step = 3                                                                   # (the step tests/test_stt_seek_kernel_gpu.py's launch takes)
    want = [F.sample_row_ts(lg[r], hists[r], T0, eos, never, begin, -1, T, F.row_hash(SEED, int(key[r]), T_INDEX, int(sample[r]), step)) for r in range(21)]
    top = leaders([SR.step_row(lg[r], hists[r], T0, eos, never, begin, -1)[0] for r in range(21)], [p for p, _ in want])
    margins = [m for _, m in want if np.isfinite(m)]
    assert all(abs(m) >= 1e-3 for m in margins) and any(m > 0 for m in margins) and any(m < 0 for m in margins)
    assert eos in top and any(t < eos for t in top) and any(t >= T0 for t in top)
    nat = model(ctx, cfg)
    try:
        state = [SR.state_of(h, T0) for h in hists]
        smp = KS.device_step(nat, lg, T, SEED, T_INDEX, key, sample, scores, step=step, ts=(-1, [s[0] for s in state], [s[1] for s in state]))
        beam = KT.device_step(nat, lg[:, None, :], 1, scores, 21, 1, [1] * 21, [0] * 21, False, -1, hists)
    finally:
        nat.close()
    assert smp["tok"].tolist() == top
    for r in range(21):
        score, row = first_candidate(beam, r, 1, top[r], eos)
        assert bits(score) == bits(smp["score"][r]), (r, score, smp["score"][r])
        if row is not None:
            assert (beam["flags"][row], beam["last"][row]) == (smp["flags"][r], smp["last"][r]) == SR.state_of(hists[r] + [top[r]], T0)


def test_the_first_step_reads_one_row_per_window(ctx):
    """row_stride 1, max_initial_timestamp_index 25: 3 windows of 4 beams / 4 samples; every sample of a window takes what the
    window's one live beam offers first."""
    cfg = SC.seek_test_config()
    eos, V, W, B = cfg.eos_id, cfg.vocab, 3, 4
    never, begin = SR.suppress_mask(cfg)
    rng = np.random.default_rng(2302)
    lg = rng.uniform(-8.0, 2.0, size=(W, V)).astype(np.float32)
    lg[:, 5], lg[:, eos], lg[:, T0 - 1], lg[:, T0 + 60] = 30.0, 29.0, 31.0, 28.0      # (barred, all four)
    lg[np.arange(W), T0 + np.array([0, 13, 25])] += 12.0
    scores = np.zeros((W, B), dtype=np.float32)
    scores[:, 0] = (-4.0 * rng.random(W)).astype(np.float32)
    key, sample = np.repeat(rng.integers(0, 1 << 20, size=W), B), np.tile(np.arange(B), W)
    want = [F.sample_row_ts(lg[r // B], [], T0, eos, never, begin, 25, T, F.row_hash(SEED, int(key[r]), T_INDEX, int(sample[r]), 0))[0] for r in range(W * B)]
    top = leaders([SR.step_row(lg[r // B], [], T0, eos, never, begin, 25)[0] for r in range(W * B)], want)
    assert top == [T0, T0, T0, T0, T0 + 13, T0 + 13, T0 + 13, T0 + 13, T0 + 25, T0 + 25, T0 + 25, T0 + 25]
    nat = model(ctx, cfg)
    try:
        smp = KS.device_step(nat, lg, T, SEED, T_INDEX, key, sample, np.repeat(scores[:, 0], B), first_step=True, step=0, samples=B, row_stride=1,
                             ts=(25, [SR.state_of([], T0)[0]] * (W * B), [0] * (W * B)))
        beam = KT.device_step(nat, lg[:, None, :], 1, scores, W, B, [1] * W, [0] * W, True, 25, [[]] * (W * B))
    finally:
        nat.close()
    assert smp["tok"].tolist() == top
    for r in range(W * B):
        score, row = first_candidate(beam, r // B, B, top[r], eos)
        assert bits(score) == bits(smp["score"][r]), (r, score, smp["score"][r])
        assert (beam["flags"][row], beam["last"][row]) == (smp["flags"][r], smp["last"][r]) == (3, top[r])


def plain_case(ctx, cfg, lg, first_step, seed):
    """Rows without the timestamp rule through both kernels, one live beam per window."""
    n, eos = len(lg), cfg.eos_id
    rng = np.random.default_rng(seed)
    scores = (-4.0 * rng.random(n)).astype(np.float32)
    key, sample = rng.integers(0, 1 << 20, size=n), rng.integers(0, 8, size=n)
    step = 0 if first_step else 3
    never, begin = R.masks(cfg)
    bad = (never | begin) if first_step else never
    rows = []
    for x in lg:
        x = x.astype(np.float64)
        x[bad] = -np.inf
        rows.append(x)
    top = leaders(rows, [F.sample_row(lg[r], bad, T, F.row_hash(SEED, int(key[r]), T_INDEX, int(sample[r]), step)) for r in range(n)])
    nat = model(ctx, cfg)
    try:
        smp = KS.device_step(nat, lg, T, SEED, T_INDEX, key, sample, scores, first_step=first_step, step=step)
        beam = KB.device_step(nat, lg[:, None, :], 1, scores, n, 1, [1] * n, [0] * n, [0] * n, first_step, step=step)
    finally:
        nat.close()
    assert smp["tok"].tolist() == top
    for r in range(n):
        score, _ = first_candidate(beam, r, 1, top[r], eos)
        assert bits(score) == bits(smp["score"][r]), (r, score, smp["score"][r])
    return top, bad


@pytest.mark.parametrize("masked", [False, True])
def test_vocabulary_300_without_the_timestamp_rule(ctx, masked):
    """8 rows; masked: a first step, so both bits of the suppress mask bind, and the largest logit of every row sits on a barred id."""
    cfg = FC.kernel_config(masked)
    rng = np.random.default_rng(2303 + int(masked))
    lg = (2.0 * rng.standard_normal((8, cfg.vocab))).astype(np.float32)
    never, begin = R.masks(cfg)
    free = np.flatnonzero(~(never | begin))
    lg[np.arange(8), rng.choice(free, size=8, replace=False)] += 14.0
    lg[0, cfg.eos_id] += 25.0 if not masked else 0.0                          # (unmasked: row 0 ends)
    if masked:
        lg[:, np.flatnonzero(never)[-1]] = 40.0
        lg[:, np.flatnonzero(begin & ~never)[0]] = 41.0
    top, bad = plain_case(ctx, cfg, lg, masked, 2305)
    assert not bad[top].any() and (masked or top[0] == cfg.eos_id)


def test_whisper_vocabulary_clamped_tail(ctx):
    """One row of 51865 ids - no multiple of the 4096 a workgroup requests per round trip: the leader on the last id the mask leaves,
    larger logits on the barred ids at the very end of the row."""
    cfg = FC.whisper_vocab_config()
    lg = (2.0 * np.random.default_rng(2306).standard_normal((1, cfg.vocab))).astype(np.float32)
    lg[0, -3:] = 30.0
    lg[0, cfg.suppress_from - 1] = 16.0
    top, _ = plain_case(ctx, cfg, lg, False, 2307)
    assert top == [cfg.suppress_from - 1]
