"""k_stt_sample_select on its own (rt_debug_stt_sample_step, rt_debug_stt_sample_step_ts) against the float64 restatement of the
sampled step (tests/stt_sample_ref.py; the inputs and margins: tests/stt_sample_cases.py): picks exact on the rows whose two
largest perturbed values are 4 (E / T + G) apart - at most 1 % of the rows may fall short, and tests/test_stt_fallback_cpu.py holds
the reference's own share below 0.5 % - new scores within E, winning values within G.  This file prints the measured G."""
import ctypes as C

import numpy as np
import pytest
import torch

from rho_tts_amd import _native
from rho_tts_amd import stt as S
from tests import stt_beam_ref as R
from tests import stt_sample_cases as FC
from tests import stt_sample_ref as F
from tests import stt_seek_cases as SC
from tests import stt_seek_ref as SR

pytestmark = pytest.mark.gpu

i32p, f32p = C.POINTER(C.c_int32), C.POINTER(C.c_float)
COMMON = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_uint64, C.c_int32, i32p, i32p, f32p, i32p, C.c_int32, C.c_int32]


@pytest.fixture(scope="module")
def ctx():
    c = _native.Context(0)
    yield c
    c.close()


def model(ctx, cfg):
    m = S.NativeSTT(ctx, cfg, {k: v.cuda() for k, v in S.synthetic_state(cfg, 789).items()})
    m.lib.rt_debug_stt_sample_step.argtypes = COMMON + [i32p, f32p, f32p, i32p, i32p]
    m.lib.rt_debug_stt_sample_step_ts.argtypes = COMMON + [C.c_int32, i32p, i32p, i32p, f32p, f32p, i32p, i32p, i32p, i32p]
    return m


@pytest.fixture(scope="module")
def nats(ctx):
    """{masked: model} at vocabulary 300, and the model with timestamps (vocabulary 400)."""
    made = {True: model(ctx, FC.kernel_config(True)), False: model(ctx, FC.kernel_config(False)), "ts": model(ctx, SC.seek_test_config())}
    yield made
    for m in made.values():
        m.close()


def device_step(nat, logits, T, seed, t_index, key, sample, scores, done=None, first_step=False, step=0, samples=1, row_stride=None, ts=None):
    """One launch over len(key) rows -> dict of per-row arrays.  ts: (max_initial, flags, last) for the timestamp instantiation."""
    n = len(key)
    d = torch.from_numpy(np.ascontiguousarray(logits, dtype=np.float32)).cuda()
    torch.cuda.synchronize()
    arr = lambda a, t: np.ascontiguousarray(a, dtype=t)
    key, sample, scores = arr(key, np.int32), arr(sample, np.int32), arr(scores, np.float32)
    done = arr(done if done is not None else np.zeros(n), np.int32)
    tok, so, val, dn, live = np.full(n, -9, np.int32), np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros(n, np.int32), C.c_int32()
    p = lambda a: a.ctypes.data_as(i32p if a.dtype == np.int32 else f32p)
    head = [nat.handle, C.c_void_p(d.data_ptr()), int(row_stride or samples), n, samples, float(T), int(seed), int(t_index), p(key), p(sample), p(scores), p(done),
            int(first_step), int(step)]
    out = dict(tok=tok, score=so, val=val, done=dn)
    if ts is None:
        nat.ctx.check(nat.lib.rt_debug_stt_sample_step(*head, p(tok), p(so), p(val), p(dn), C.byref(live)), "rt_debug_stt_sample_step")
    else:
        fl_in, lt_in = arr(ts[1], np.int32), arr(ts[2], np.int32)
        fl, lt = np.zeros(n, np.int32), np.zeros(n, np.int32)
        nat.ctx.check(nat.lib.rt_debug_stt_sample_step_ts(*head, int(ts[0]), p(fl_in), p(lt_in), p(tok), p(so), p(val), p(dn), C.byref(live), p(fl), p(lt)),
                      "rt_debug_stt_sample_step_ts")
        out.update(flags=fl, last=lt)
    out["live"] = live.value
    return out


def bad_ids(cfg, first_step):
    never, begin = R.masks(cfg)
    return (never | begin) if first_step else never


def hold(case, got, bad, eos, worst):
    """The device's rows against the reference's: picks exact where decisive, scores within E, winning values within G."""
    tok, lp, val, gap = FC.reference_rows(case, bad)
    ok = gap >= FC.gap_bound(case["T"])
    skipped = 1.0 - ok.mean()
    assert skipped <= FC.SKIP_SHARE_DEVICE, skipped
    assert np.array_equal(got["tok"][ok], tok[ok])
    same = got["tok"] == tok
    err_s = np.abs(got["score"][same].astype(np.float64) - (case["scores"][same].astype(np.float64) + lp[same]))
    err_v = np.abs(got["val"][same].astype(np.float64) - val[same])
    worst["score"], worst["val"] = max(worst["score"], err_s.max()), max(worst["val"], err_v.max())
    print(f"T {case['T']} rows {len(tok)}: skipped {skipped:.4%}, max |score - reference| {err_s.max():.3g}, max |winning value - reference| {err_v.max():.3g}")
    assert err_s.max() <= FC.E and err_v.max() <= FC.G
    assert np.array_equal(got["done"], (got["tok"] == eos).astype(np.int32)) and got["live"] == int((got["tok"] != eos).sum())
    return tok


@pytest.mark.parametrize("masked", [False, True])
def test_4096_rows_in_one_launch(nats, masked):
    nat, worst = nats[masked], dict(score=0.0, val=0.0)
    bad = bad_ids(nat.cfg, masked)
    for T in FC.TEMPERATURES:
        case = FC.kernel_case(T, masked)
        got = device_step(nat, case["logits"], T, case["seed"], case["t_index"], case["key"], case["sample"], case["scores"], first_step=case["first_step"], step=case["step"])
        tok = hold(case, got, bad, nat.cfg.eos_id, worst)
        assert not bad[tok].any() and len(set(tok.tolist())) > 100          # (a draw, not an arg-max)
    print("G measured (V = 300)", worst["val"], "recorded", FC.G, "| score error", worst["score"], "E", FC.E)


def test_whisper_vocabulary_clamped_tail(ctx):
    """51865 ids: no multiple of the 4096 a workgroup requests per round trip, so the last round's clamped loads are exercised."""
    cfg = FC.whisper_vocab_config()
    nat, worst = model(ctx, cfg), dict(score=0.0, val=0.0)
    try:
        for case in FC.whisper_vocab_cases():
            first = case["first_step"]
            got = device_step(nat, case["logits"], case["T"], case["seed"], case["t_index"], case["key"], case["sample"], case["scores"], first_step=first, step=case["step"])
            tok = hold(case, got, bad_ids(cfg, first), cfg.eos_id, worst)
            assert (tok <= cfg.eos_id).all()
        print("G measured (V = 51865)", worst["val"])
    finally:
        nat.close()


def test_nan_logits_a_lone_survivor_and_rows_that_are_done(nats):
    nat = nats[True]
    cfg, V = nat.cfg, nat.cfg.vocab
    eos = cfg.eos_id
    case = FC.kernel_case(0.6, False, rows=4, V=V)
    case["first_step"], case["step"] = False, 5
    lg = case["logits"]
    lg[0, ::3] = np.nan                                                    # row 0: NaNs scattered, the largest values among them
    lg[0, 1::3] -= 4.0
    lg[1, :] = -np.inf                                                     # row 1: end-of-sequence is the only survivor
    lg[1, eos] = -2.5
    lg[1, 295] = 50.0                                                      # (suppressed)
    done = [0, 0, 1, 0]                                                    # row 2 comes in done
    got = device_step(nat, lg, 0.6, case["seed"], case["t_index"], case["key"], case["sample"], case["scores"], done=done, step=5)
    tok, lp, val, gap = FC.reference_rows(case, bad_ids(cfg, False))
    assert gap[0] >= FC.gap_bound(0.6) and gap[3] >= FC.gap_bound(0.6)
    assert got["tok"][0] == tok[0] and tok[0] % 3 != 0 and np.isfinite(got["score"][0]) and abs(got["score"][0] - (case["scores"][0] + lp[0])) <= FC.E
    assert got["tok"][1] == eos and got["done"][1] == 1 and abs(got["score"][1] - case["scores"][1]) <= FC.E          # log-probability 0
    # the row that came in done: nothing written (the pick keeps the -1 the entry point puts there), score bit for bit
    assert got["tok"][2] == -1 and got["done"][2] == 1 and got["score"][2].tobytes() == case["scores"][2].tobytes()
    assert got["tok"][3] == tok[3] and got["live"] == 2


# the history shapes of tests/test_stt_seek_kernel_gpu.py behind the first step, and what each allows
T0, EOS_TS = SC.TIMESTAMP_BEGIN, SC.seek_test_config().eos_id
SHAPES = [[T0 + 7], [T0 + 7, 31], [T0 + 3, 31, T0 + 20, T0 + 20], [T0 + 3, 31, T0 + 20, T0 + 20, 44, 45], [T0, 12, 13, T0 + 50],
          [T0 + 1, 9, T0 + 5, T0 + 5, 8, T0 + 30, T0 + 30], [T0 + 2, 31, 32, 33]]


def ts_rows(T, hists, first_step, max_initial, seed):
    """Rows under the timestamp rule with a per-row offset on the timestamp ids, so that the logsumexp rule decides both ways: the
    first seed from `seed` on whose picks and logsumexp decisions are all decisive."""
    cfg = SC.seek_test_config()
    never, begin = SR.suppress_mask(cfg)
    n = len(hists)
    for s in range(seed, seed + 200):
        case = FC.kernel_case(T, False, rows=n, V=cfg.vocab, seed=s)
        case["first_step"], case["step"] = first_step, 0 if first_step else 4
        for r in range(n):
            case["logits"][r, T0:] += (-6.0, 0.0, 7.0)[(r + s) % 3]
        want = []
        for r in range(n):
            rh = F.row_hash(case["seed"], int(case["key"][r]), case["t_index"], int(case["sample"][r]), case["step"])
            want.append(F.sample_row_ts(case["logits"][r], hists[r], T0, cfg.eos_id, never, begin, max_initial, T, rh))
        if all(p.gap >= FC.gap_bound(T) and abs(m) >= 1e-3 for p, m in want):
            return case, want
    raise AssertionError("no seed gives decisive rows")


@pytest.mark.parametrize("T", [0.2, 1.0])
def test_the_timestamp_instantiation(nats, T):
    nat = nats["ts"]
    # every history shape twice (two offsets of the timestamp ids), behind the first step
    hists = SHAPES + SHAPES
    case, want = ts_rows(T, hists, False, -1, 300)
    state = [SR.state_of(h, T0) for h in hists]
    got = device_step(nat, case["logits"], T, case["seed"], case["t_index"], case["key"], case["sample"], case["scores"], step=case["step"],
                      ts=(-1, [s[0] for s in state], [s[1] for s in state]))
    assert got["tok"].tolist() == [p.tok for p, _ in want]
    assert [(int(a), int(b)) for a, b in zip(got["flags"], got["last"])] == [SR.state_of(h + [p.tok], T0) for h, (p, _) in zip(hists, want)]
    assert np.abs(got["score"] - (case["scores"] + np.array([p.lp for p, _ in want]))).max() <= FC.E
    lse = [m for _, m in want if np.isfinite(m)]
    assert any(m > 0 for m in lse) and any(m < 0 for m in lse)               # timestamps win in some rows and lose in others
    assert all(p.tok >= T0 for p, m in want if m > 0)
    # behind a pair: text only; closing a pair: a timestamp (not below the last) or the end; non-decreasing otherwise
    for h, (p, _) in zip(hists, want):
        flags, last = SR.state_of(h, T0)
        assert not (flags == 3 and p.tok >= T0) and not (flags == 1 and p.tok < EOS_TS) and not (p.tok >= T0 and p.tok < last)
    # the first step: one row of logits per window (row_stride 1) read by 4 samples each, a timestamp of at most max_initial
    windows = 3
    case, _ = ts_rows(T, [[]] * windows, True, 25, 500)
    case["logits"][:, 5], case["logits"][:, EOS_TS], case["logits"][:, T0 - 1], case["logits"][:, T0 + 60] = 30.0, 29.0, 31.0, 28.0
    never, begin = SR.suppress_mask(nat.cfg)
    keys, samples = np.repeat(case["key"], 4), np.tile(np.arange(4), windows)
    got = device_step(nat, case["logits"], T, case["seed"], case["t_index"], keys, samples, np.zeros(4 * windows), first_step=True, step=0, samples=4, row_stride=1,
                      ts=(25, [0] * (4 * windows), [0] * (4 * windows)))
    for r in range(4 * windows):
        p, _ = F.sample_row_ts(case["logits"][r // 4], [], T0, nat.cfg.eos_id, never, begin, 25, T, F.row_hash(case["seed"], int(keys[r]), case["t_index"], r % 4, 0))
        if p.gap >= FC.gap_bound(T):
            assert got["tok"][r] == p.tok and abs(got["score"][r] - p.lp) <= FC.E
        assert T0 <= got["tok"][r] <= T0 + 25 and (got["flags"][r], got["last"][r]) == (3, got["tok"][r])


def test_a_row_does_not_depend_on_the_launch(nats):
    """The same row - logits, key, sample index, score - in launches of 1, 7 and 32 rows: pick, score and winning value bit for bit."""
    nat = nats[True]
    case = FC.kernel_case(0.6, False, rows=32, V=nat.cfg.vocab, seed=77)
    seen = []
    for n, at in ((1, 0), (7, 4), (32, 19)):
        order = [k for k in range(32) if k != 5][:n]
        order[at] = 5                                                          # row 5 of the case sits at position `at`
        got = device_step(nat, case["logits"][order], 0.6, case["seed"], case["t_index"], case["key"][order], case["sample"][order], case["scores"][order], step=2)
        seen.append((int(got["tok"][at]), got["score"][at].tobytes(), got["val"][at].tobytes()))
    assert seen[0] == seen[1] == seen[2]
