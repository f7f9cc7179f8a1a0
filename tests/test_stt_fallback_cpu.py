"""The temperature fallback on the CPU: the compression ratios against their sources, the restated rule branch by branch, the
reference sampler's distribution, the generator's range, and the margins tests/stt_sample_cases.py records."""
import zlib

import numpy as np
import pytest
import torch

from rho_tts_amd import validation as V
from tests import stt_beam_ref as R
from tests import stt_sample_cases as FC
from tests import stt_sample_ref as F


def test_compression_ratio_ids_is_transformers():
    from transformers.models.whisper.generation_whisper import WhisperGenerationMixin as W
    rng = np.random.default_rng(3)
    for vocab in (300, 51865):
        for n in (1, 2, 7, 40, 224):
            ids = rng.integers(0, vocab, size=n)
            assert V.compression_ratio_ids(ids.tolist(), vocab) == W._retrieve_compression_ratio(torch.from_numpy(ids), vocab)
        loop = [11, 12, 13] * 200                                  # a phrase repeated to the token limit compresses well
        got = V.compression_ratio_ids(loop, vocab)
        assert got == W._retrieve_compression_ratio(torch.tensor(loop), vocab) and got > 2.4
    assert V.compression_ratio_ids([5], 300) == 2 / len(zlib.compress(b"\x05\x00"))          # 300 ids: two bytes each


def test_compression_ratio_text():
    s = "the quick brown fox jumps over the lazy dog"
    assert V.compression_ratio_text(f"  {s}\n") == len(s) / len(zlib.compress(s.encode()))
    loop = "so it goes. " * 60
    raw = loop.strip().encode("utf-8")
    assert V.compression_ratio_text(loop) == len(raw) / len(zlib.compress(raw)) > 2.4
    assert V.compression_ratio_text("héllo") == 6 / len(zlib.compress("héllo".encode("utf-8")))          # bytes, not characters


def test_needs_fallback_branch_by_branch():
    nan = float("nan")
    # ratio only
    assert V.needs_fallback(2.5, -0.2) and not V.needs_fallback(2.4, -0.2) and not V.needs_fallback(2.5, -0.2, compression_ratio_threshold=None)
    assert not V.needs_fallback(None, -0.2)
    # log-probability only
    assert V.needs_fallback(1.0, -1.01) and not V.needs_fallback(1.0, -1.0) and not V.needs_fallback(1.0, -1.01, logprob_threshold=None)
    # the silence exemption: both thresholds set, no-speech above its own and the average below its own
    assert not V.needs_fallback(9.0, -1.5, 0.7, no_speech_threshold=0.6)
    assert V.needs_fallback(9.0, -1.5, 0.5, no_speech_threshold=0.6) and V.needs_fallback(9.0, -0.5, 0.7, no_speech_threshold=0.6)
    assert V.needs_fallback(9.0, -1.5, 0.7, logprob_threshold=None, no_speech_threshold=0.6) and V.needs_fallback(9.0, -1.5, nan, no_speech_threshold=0.6)
    assert V.needs_fallback(9.0, -1.5, 0.7)                       # (no no-speech threshold: no exemption)


def test_pick_attempt_when_every_temperature_failed():
    # some within the compression threshold: the largest average among THOSE
    assert V.pick_attempt([(9.0, -0.1), (2.0, -1.4), (1.5, -1.2), (9.0, -0.05)]) == 2
    # none within it: the largest average among all
    assert V.pick_attempt([(9.0, -0.4), (3.0, -0.3), (5.0, -0.35)]) == 1
    # ties go to the earliest attempt
    assert V.pick_attempt([(1.0, -1.5), (1.0, -1.2), (1.0, -1.2)]) == 1 and V.pick_attempt([(9.0, -2.0), (9.0, -2.0)]) == 0
    # no ratio (no callback) is within any threshold
    assert V.pick_attempt([(None, -1.5), (None, -1.1)]) == 1 and V.pick_attempt([(9.0, -0.1), (2.0, -1.4)], compression_ratio_threshold=None) == 0


def test_the_fallback_loop_of_the_reference():
    """tests/stt_sample_ref.py fallback on scripted attempts: stops at the first attempt that needs no other, else pick_attempt."""
    A = lambda avg, n=3: F.Attempt(list(range(n)), avg * (n + 1), 0.0, None, 0.0, 1.0)
    ret = iter(F.script([[2]], 3))
    fb = F.fallback(lambda: A(-0.5), lambda T, t: A(-0.6 - t), (0.0, 0.4, 0.8), list, lambda ids: next(ret))
    assert fb.chosen == 2 and [a.ratio for a in fb.attempts] == [9.0, 9.0, 1.0] and [a.temperature for a in fb.attempts] == [0.0, 0.4, 0.8]
    ret = iter(F.script([[3]], 3))
    fb = F.fallback(lambda: A(-0.5), lambda T, t: A(-0.6 + 0.2 * t), (0.0, 0.4, 0.8), list, lambda ids: next(ret))
    assert fb.chosen == 2 and len(fb.attempts) == 3 and fb.pick_margin == pytest.approx(0.2)          # (averages -0.5, -0.4, -0.2)
    fb = F.fallback(lambda: A(-1.5), lambda T, t: A(-0.2), (0.0, 0.4), list, None)
    assert fb.chosen == 1 and fb.threshold_margin == pytest.approx(0.5)
    fb = F.fallback(lambda: A(-1.5), lambda T, t: A(-0.2), (0.0, 0.4), list, None, no_speech_prob=0.9, no_speech_threshold=0.6)
    assert fb.chosen == 0 and len(fb.attempts) == 1
    assert F.script([[1, 0, 2], [3]], 3) == [9.0, 1.0, 9.0, 1.0, 9.0, 1.0, 9.0, 9.0, 9.0]


CHI_SEED = 20240611          # the seed of the distribution test; the p-values it gives are asserted below


@pytest.mark.parametrize("T", [0.2, 1.0])
def test_the_reference_sampler_draws_from_the_tempered_softmax(T):
    """65536 draws (distinct step counters) at V = 300: chi-square over the ids, pooled in descending probability to an expected count
    of at least 5, against softmax(x / T) over the surviving ids.  p = 0.71 at T = 0.2 (22 pools) and 0.032 at T = 1.0 (271 pools) at this seed."""
    from scipy.stats import chi2
    n, Vn = 65536, 300
    rng = np.random.default_rng(CHI_SEED)
    x = rng.standard_normal(Vn) * 2.0
    bad = np.zeros(Vn, dtype=bool)
    bad[290:] = True
    bad[7] = True
    x[11] = np.nan
    rh = np.array([F.row_hash(CHI_SEED, 17, 1, 3, step) for step in range(n)], dtype=np.uint64)
    alive = np.flatnonzero(~bad & ~np.isnan(x))
    v = x[alive][None, :] / T + F.gumbel(rh[:, None], alive[None, :])
    picks = alive[np.argmax(v, axis=1)]
    p = np.exp(x[alive] / T - (x[alive] / T).max())
    p /= p.sum()
    order = np.argsort(-p)
    counts = np.bincount(picks, minlength=Vn)[alive][order].astype(np.float64)
    expect = p[order] * n
    pooled_c, pooled_e, c_acc, e_acc = [], [], 0.0, 0.0
    for c, e in zip(counts, expect):
        c_acc, e_acc = c_acc + c, e_acc + e
        if e_acc >= 5.0:
            pooled_c.append(c_acc); pooled_e.append(e_acc)
            c_acc = e_acc = 0.0
    pooled_c[-1] += c_acc
    pooled_e[-1] += e_acc
    stat = float(((np.array(pooled_c) - np.array(pooled_e)) ** 2 / np.array(pooled_e)).sum())
    pv = float(chi2.sf(stat, len(pooled_e) - 1))
    print(f"T {T}: {len(pooled_e)} pools, chi-square {stat:.1f}, p {pv:.3g}")
    assert len(pooled_e) >= (5 if T < 0.5 else 50) and pv > 1e-4


def test_a_vanishing_temperature_is_the_masked_arg_max():
    rng = np.random.default_rng(5)
    never, begin = R.masks(FC.kernel_config(True))
    for k in range(64):
        x = rng.standard_normal(300) * 2.0
        x[rng.integers(0, 300)] = np.nan
        x[295] = 40.0                                               # (suppressed)
        bad = (never | begin) if k % 2 else never
        p = F.sample_row(x, bad, 1e-3, F.row_hash(9, k, 0, 0, k))
        want = np.where(bad | np.isnan(x), -np.inf, x)
        assert p.tok == int(np.argmax(want)) and not bad[p.tok]


def test_u_never_reaches_0_or_1():
    k = np.arange(1 << 23, dtype=np.int64)
    u = F.u_of_k(k)
    assert u.min() == 2.0 ** -24 and u.max() == 1.0 - 2.0 ** -24
    u32 = (k.astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -23)          # the device's arithmetic: exact
    assert u32.dtype == np.float32 and np.array_equal(u32.astype(np.float64), u)
    g = -np.log(-np.log(u[[0, -1]]))
    assert np.isfinite(g).all() and g[0] < -2.8 and g[1] > 16.6
    # 24 bits would not do: (2^24 - 1) + 0.5 rounds to 2^24 in float32
    assert np.float32(2 ** 24 - 1) + np.float32(0.5) == np.float32(2 ** 24)
    # the counter is the top 23 bits of the hash
    assert int(F.counter_k(0xDEADBEEF, 12345)) == int(F.mix32((0xDEADBEEF + 12345 * 0x85EBCA77) & F.M32)) >> 9 < (1 << 23)


def test_the_row_hash_is_the_chain_of_the_talkers_generator():
    """rt_uniform's chain (oracle/sampling.py) extended by one link: with temperature index and step in the places of frame and group
    the first four links are that function's hash."""
    from oracle import sampling as OS
    a = OS.mix32((0x1234567887654321 & F.M32) ^ 0x85EBCA6B)
    b = OS.mix32(a + 41 * 0x9E3779B1)
    c = OS.mix32(b + 2 * 0x85EBCA77)
    d = OS.mix32(c + 3 * 0xC2B2AE3D + (0x1234567887654321 >> 32))
    assert F.row_hash(0x1234567887654321, 41, 2, 3, 7) == OS.mix32(d + 7 * 0x9E3779B1)
    assert len({F.row_hash(1, k, t, j, s) for k in range(3) for t in range(3) for j in range(3) for s in range(3)}) == 81


def test_the_kernel_tests_rows_are_decisive():
    """The share of rows tests/test_stt_sample_kernel_gpu.py may skip for lack of margin is 1 %; the reference alone must stay below
    0.5 % (about 0.1 % is expected at T = 1 and less below)."""
    for masked in (False, True):
        cfg = FC.kernel_config(masked)
        never, begin = R.masks(cfg)
        bad = (never | begin) if masked else never
        for T in FC.TEMPERATURES:
            case = FC.kernel_case(T, masked)
            tok, lp, val, gap = FC.reference_rows(case, bad)
            share = float((gap < FC.gap_bound(T)).mean())
            print(f"masked {masked} T {T}: {share:.4%} of {len(tok)} rows below {FC.gap_bound(T):.3g}")
            assert share <= FC.SKIP_SHARE_REFERENCE and not bad[tok].any() and np.abs(val).max() < 64.0
            k = 17                                                  # the vectorised reference is the row-by-row one
            p = F.sample_row(case["logits"][k], bad, T, F.row_hash(case["seed"], int(case["key"][k]), case["t_index"], int(case["sample"][k]), case["step"]))
            assert (p.tok, p.lp, p.val, p.gap) == pytest.approx((tok[k], lp[k], val[k], gap[k]), rel=1e-12)
    cfg = FC.whisper_vocab_config()                                 # the 8-row launches at 51865 ids: no row may be skipped
    never, begin = R.masks(cfg)
    for case in FC.whisper_vocab_cases():
        tok, lp, val, gap = FC.reference_rows(case, (never | begin) if case["first_step"] else never)
        assert (gap >= FC.gap_bound(case["T"])).all() and (tok <= cfg.eos_id).all() and np.abs(val).max() < 64.0
        assert case["first_step"] or tok[0] == cfg.suppress_from - 1          # (the planted last id the mask leaves)
    assert FC.gap_bound(1.0) == 4 * (FC.E + FC.G) and FC.MARGIN == 4 * FC.E


@pytest.fixture(scope="module")
def oracle_a():
    from oracle import whisper as OW
    return OW.build(FC.CFG, FC.STATES["A"](FC.CFG))


def test_every_recorded_case_has_its_margin(oracle_a):
    """The end-to-end cases of tests/test_stt_fallback_gpu.py on the CPU reference: every attempt of every case - forced through all
    three temperatures, which covers the scripts that stop earlier - is decisive, and the recorded figures are what the reference gives."""
    from tests import stt_beam_cases as K
    from tests import stt_seek_cases as SC
    cfg = FC.CFG
    for st, cl, margin, gap, pick in FC.EX_CASES:
        mel = R.window_mels(cfg, K.CLIPS[cl](), FC.SR)[0]
        fb = F.window_fallback(oracle_a, cfg, mel, FC.BEAM, FC.BEST_OF, FC.TEMPS, FC.SEED, 0, ratio=lambda ids: 9.0, logprob_threshold=None)
        assert len(fb.attempts) == 3 and F.decisive(fb, FC.E, FC.G, FC.MARGIN), (cl, fb)
        got = (min(a.margin for a in fb.attempts), min(a.gap for a in fb.attempts), fb.pick_margin)
        print(cl, got)
        assert got == pytest.approx((margin, gap, pick), rel=0.02) and all(len(a.ids) > 0 for a in fb.attempts)
        assert got[0] >= FC.MARGIN and all(a.gap >= FC.gap_bound(a.temperature) for a in fb.attempts[1:]) and pick >= FC.MARGIN
    o = FC.LOGPROB_CASE
    mel = R.window_mels(cfg, K.CLIPS[o["clip"]](), FC.SR)[0]
    for thr, attempts, chosen in ((o["passes"], 1, 0), (o["fails"], 3, 0)):
        fb = F.window_fallback(oracle_a, cfg, mel, FC.BEAM, FC.BEST_OF, FC.TEMPS, FC.SEED, 0, logprob_threshold=thr)
        assert (len(fb.attempts), fb.chosen) == (attempts, chosen) and F.decisive(fb, FC.E, FC.G, FC.MARGIN) and fb.threshold_margin >= 0.2
    st, cl, mi, plain_offsets, offsets = FC.SEEK_CASE
    tick = int(0.02 * FC.SR)
    for B in (1, 5):
        for returns, want in (([], plain_offsets), ([1.0, 9.0], offsets)):
            ret = iter(returns + [1.0] * 16)
            wins = F.clip_fallback_seek(oracle_a, cfg, SC.CLIPS[cl](), FC.SR, B, FC.BEST_OF, FC.TEMPS, FC.SEED, lambda ids: next(ret), mi, logprob_threshold=None)
            assert [w.offset // tick for w in wins] == want and all(F.decisive(w.fb, FC.E, FC.G, FC.MARGIN) for w in wins)
            assert [len(w.fb.attempts) for w in wins] == ([1, 2, 1] if returns else [1, 1, 1])
    # the scripts of two and of every failed attempt through the seek loop: offsets, attempts and choices as recorded, all decisive
    for cl, ks, per in FC.SEEK_SCRIPTS:
        for B, (offs, attempts, chosen) in per.items():
            ret = iter(F.script([[k] for k in ks], len(FC.TEMPS)) + [1.0] * 16)
            asked = []
            wins = F.clip_fallback_seek(oracle_a, cfg, SC.CLIPS[cl](), FC.SR, B, FC.BEST_OF, FC.TEMPS, FC.SEED, lambda ids: asked.append(ids) or next(ret),
                                        FC.SEEK_MAX_INITIAL, logprob_threshold=None)
            assert ([w.offset // tick for w in wins], [len(w.fb.attempts) for w in wins], [w.fb.chosen for w in wins]) == (offs, attempts, chosen), (cl, ks, B)
            assert all(F.decisive(w.fb, FC.E, FC.G, FC.MARGIN) for w in wins) and len(asked) == sum(attempts) and all(asked)
            assert all(t < cfg.timestamp_begin for ids in asked for t in ids)
        assert 2 in {c for _, (_, a, ch) in per.items() for c, n in zip(ch, a) if n == 3}          # (temperature index 2 stands somewhere)


def test_the_whisper_tiny_case_is_decisive():
    """The case tests/test_stt_fallback_gpu.py holds unconditionally at Whisper-tiny dimensions, on the CPU reference."""
    o = FC.TINY_CASE
    cfg, state, x, fb = FC.tiny_reference()
    assert len(fb.attempts) == 2 and fb.chosen == 1 and F.decisive(fb, FC.E, FC.G, FC.MARGIN) and fb.result.ids
    got = (fb.attempts[0].margin, fb.attempts[1].margin, fb.attempts[1].gap)
    print(got)
    assert got == pytest.approx((o["margin_beam"], o["margin_best_of"], o["gap"]), rel=0.02)
    assert got[0] >= FC.MARGIN and got[1] >= FC.MARGIN and got[2] >= FC.gap_bound(0.4)
