"""CPU checks of tests/encoder_ref.py: the references agree with oracle/encoder.py (itself pinned to transformers' Mimi in
tests/test_oracle_encoder.py), the shared inputs have the properties the GPU tests rely on, and every comparison of
tests/test_encoder_kernels_gpu.py rejects a reference with ONE minimal defect - so a kernel with that defect could not pass."""
import numpy as np
import pytest
import torch

from oracle import encoder as E
from rho_tts_amd import config, weights
from tests import encoder_ref as R
from tests import rowops_ref as RR

F64 = torch.float64


def rejects(fn, *args, **kw):
    with pytest.raises(AssertionError):
        fn(*args, **kw)


def g(seed):
    return np.random.default_rng(seed)


# ------------------------------------------------------------------------------------------ against the oracle
@pytest.mark.parametrize("K", [1, 2, 7, 9])
def test_conv0_reference_matches_oracle_causal_conv(K):
    T, C = 23, 16
    pcm, w, b = (g(1).standard_normal(n).astype(np.float32) for n in (T, (C, K), C))
    want = E.causal_conv(torch.from_numpy(pcm).to(F64).reshape(1, 1, -1), torch.from_numpy(w).to(F64)[:, None, :], torch.from_numpy(b).to(F64))[0].T
    ref = R.conv0_ref(pcm, w, b)
    assert np.abs(ref - want.numpy()).max() < 1e-14
    # the float32 mirror is the same sum rounded: within (K + 1) u of the float64 one, and exactly it on integer-valued data
    mag = R.conv0_ref(np.abs(pcm), np.abs(w), np.abs(b))
    assert (np.abs(R.conv0_ref(pcm, w, b, mirror=True) - ref) <= (K + 1) * R.U24 * mag).all()
    ip, iw, ib = (g(2).integers(-4, 5, n).astype(np.float32) for n in (T, (C, K), C))
    R.assert_equal(R.conv0_ref(ip, iw, ib, mirror=True), R.conv0_ref(ip, iw, ib).astype(np.float32))


def test_elu_planes_reference_matches_torch_elu_and_its_bound_holds_for_float32():
    x = torch.from_numpy((3 * g(3).standard_normal((50, 16))).astype(np.float32))
    hi, lo, e64 = R.elu_planes_ref(x)
    assert float((e64 - torch.nn.functional.elu(x.to(F64))).abs().max()) < 1e-15
    assert bool(((hi.float() + lo.float()).to(F64) - e64).abs().le(R.elu_neg_tol(e64)).all())          # the CPU's own expm1f passes
    pos = x >= 0
    assert torch.equal(hi[pos], x[pos].to(torch.bfloat16))


def test_rvq_reference_equals_oracle_level_by_level():
    cfg = config.tiny()
    W = {k: v.float() for k, v in weights.synthetic_state(cfg, 789).items() if k.startswith("enc.vq.")}
    emb = torch.from_numpy(g(4).standard_normal((37, cfg.codec.enc_hidden)).astype(np.float32))
    want = E.rvq_encode(W, cfg, emb).numpy()
    sem = (emb @ W["enc.vq.semantic.input_proj.weight"].T).numpy()
    aco = (emb @ W["enc.vq.acoustic.input_proj.weight"].T).numpy()
    cbs = [W[f"enc.vq.codebook.{q}"].numpy() for q in range(cfg.codec.num_quantizers)]
    codes, res = R.rvq_ref(sem, aco, cbs)
    assert np.array_equal(codes, want)
    r = aco.copy()
    for q in range(1, len(cbs)):                                   # level by level, residual by residual
        assert np.array_equal(codes[:, q], E.rvq_level(r, cbs[q]))
        r = (r - cbs[q][codes[:, q]]).astype(np.float32)
    R.assert_equal(res, r)
    c1, r1 = R.rvq_ref(sem, aco, cbs[:1])                          # Q == 1: no acoustic level, the residual is aco itself
    assert np.array_equal(c1[:, 0], want[:, 0])
    R.assert_equal(r1, aco)


def test_stats_pool_and_gemv_references_match_oracle_speaker_head():
    cfg = config.tiny()
    W = {k: v.float() for k, v in weights.synthetic_state(cfg, 789).items() if k.startswith("enc.spk.")}
    feats = torch.from_numpy(g(5).standard_normal((21, cfg.codec.enc_hidden)).astype(np.float32))
    st = R.stats_pool_ref(feats)
    h, _ = R.gemv_ref(W["enc.spk.fc1.weight"], W["enc.spk.fc1.bias"], st, True)
    y, mag = R.gemv_ref(W["enc.spk.fc2.weight"], W["enc.spk.fc2.bias"], h, False)
    want = E.speaker_embed({k: v.to(F64) for k, v in W.items()}, cfg, feats.to(F64))
    assert float((y - want).abs().max()) < 1e-13 and bool((mag >= y.abs() - 1e-13).all())
    # the float32 mirror of the pooling sits inside the derived bound
    m = torch.from_numpy(R.stats_pool_mirror(feats.numpy())).to(F64)
    tm, ts = R.stats_pool_tol(feats)
    C = feats.shape[1]
    assert bool((m[:C] - st[:C]).abs().le(tm).all()) and bool((m[C:] - st[C:]).abs().le(ts).all())


def test_stage_references_match_the_oracle_and_its_float32_error_sits_inside_the_bounds():
    cfg = config.tiny()
    W = {k: v.float() for k, v in weights.synthetic_state(cfg, 789).items() if k.startswith("enc.")}
    n = 9 * cfg.codec.total_upsample
    pcm = (0.3 * np.sin(np.arange(n) / 17.0) + 0.05 * g(6).standard_normal(n)).astype(np.float32)
    codes, spk, mid = E.encode(W, cfg, pcm, return_intermediates=True)
    feats, bound = R.seanet_ref(W, cfg, pcm)
    err = (mid["feats"].to(F64) - feats).abs().reshape(-1)
    idx = R.feats_check_indices(err, feats.shape)
    fb = bound(idx)
    assert bool((err[idx] <= fb).all()) and float(err.max()) <= float(fb.max()) < 0.05 * float(feats.abs().max())
    emb, eb = R.downsample_ref(W, mid["tf"])
    assert float((mid["emb"].to(F64) - emb).abs().max()) < 1e-5 * float(emb.abs().max())
    sem, sb = R.projection_ref(W, mid["emb"], "semantic")
    want = mid["emb"] @ W["enc.vq.semantic.input_proj.weight"].T
    assert float((want.to(F64) - sem).abs().max()) < 1e-5 * float(sem.abs().max())
    # a lo plane dropped from the operand (8 bits instead of 16) breaks the bounds of the exact-input stages
    tf_hi = mid["tf"].to(torch.bfloat16).float()
    bad, _ = R.downsample_ref(W, tf_hi)
    rejects(RR.check_close, bad, emb, eb)
    bad, _ = R.projection_ref(W, mid["emb"].to(torch.bfloat16).float(), "semantic")
    rejects(RR.check_close, bad, sem, sb)


# ------------------------------------------------------------------------------------------ the shared quantiser inputs
def test_integer_case_ties_are_exact_and_every_planted_pattern_decides_a_code():
    for (T, D, K, Q) in ((33, 9, 3000, 5), (3, 1, 4096, 2), (9, 17, 37, 1)):
        sem, aco, cbs, planted = R.rvq_int_case(T, D, K, Q, seed=11)
        codes, res = R.rvq_ref(sem, aco, cbs)
        x = aco.copy()
        for q in range(Q):
            xin = sem if q == 0 else x
            d32, d64 = R.rvq_distances(xin, cbs[q]), R.rvq_distances(xin, cbs[q], f64=True)
            assert np.array_equal(d32.astype(np.float64), d64)                       # exact: the order cannot matter
            assert np.array_equal(R.rvq_level_ref(xin, cbs[q], order="desc"), codes[:, q])
            has = [t for t in range(T) if planted[q][t]]
            assert len(has) >= min(T, K // 4)
            n = min(2, D)
            for t in has:                                                              # every planted position ties with its twin
                assert (d64[t, list(planted[q][t])] == n).all()
            if D >= 9:             # (few dimensions tie by themselves; another frame's planted entry may come closer now and then)
                tied = [(d64[t] == d64[t].min()).sum() >= 2 for t in has if len(planted[q][t]) >= 2]                # the minimum is attained twice: the index decides
                assert tied and np.mean(tied) >= 0.5
                if q <= 1:         # (fresh vectors; the residuals of later levels are a few units, close to each other's entries)
                    decided = [d64[t].min() == n and codes[t, q] == min(planted[q][t]) for t in has]
                    assert np.mean(decided) >= 0.5                                     # ... and the lowest index takes the code
            if q >= 1:
                x = (x - cbs[q][codes[:, q]]).astype(np.float32)
    pats = R.rvq_tie_positions(4096)
    assert {(5, 1029), (130, 137), (3, 195), (0, 2048), (4095,), (4032, 4095)} <= set(pats)
    assert R.rvq_tie_positions(37)[:3] == [(5,), (9,), (3,)] and (0, 36) in R.rvq_tie_positions(37)


def test_census_case_plants_the_targets():
    for (T, D, K, Q) in ((33, 8, 3000, 5), (3, 1, 4096, 2), (2, 7, 1025, 5), (5, 40, 37, 2), (4, 4, 4096, 5)):
        sem, aco, cbs, target = R.rvq_census_case(T, D, K, Q, seed=12)
        codes, res = R.rvq_ref(sem, aco, cbs)
        assert np.array_equal(codes, target)
        if Q > 1:
            assert not res.any()                                                       # everything planted has been taken off again
        assert set(target[0]) == {0} and set(target[-1]) == {K - 1}


@pytest.mark.parametrize("case,floor", [(R.NEAR_TIE, 5), (R.NEAR_TIE_2, 5)])
def test_near_tie_case_turns_on_the_evaluation_order(case, floor):
    """On this input a fused multiply-add, a descending sum and float64 distances each change codes against oracle rvq_level
    (numpy 2.x: 8, 24 and 19 frames of 33; 15, 34 and 35 of 64) - so exact equality on the GPU pins the order, not only the argmin."""
    x, cb = R.rvq_near_tie_case(**case)
    want = E.rvq_level(x, cb)
    assert np.array_equal(R.rvq_level_ref(x, cb), want)
    for kw in (dict(fma=True), dict(order="desc"), dict(f64=True)):
        flips = int((R.rvq_level_ref(x, cb, **kw) != want).sum())
        print(case["K"], kw, flips)
        assert flips >= floor, (kw, flips)
        rejects(R.assert_equal, R.rvq_level_ref(x, cb, **kw), want)


# ------------------------------------------------------------------------------------------ one minimal defect each
def test_exact_comparison_rejects_each_quantiser_defect():
    sem, aco, cbs, planted = R.rvq_int_case(33, 9, 3000, 5, seed=11)
    codes, res = R.rvq_ref(sem, aco, cbs)
    for defect in ("highest", "no_last_entry", "wrong_level"):
        c, r = R.rvq_ref(sem, aco, cbs, defect=defect)
        rejects(R.assert_equal, c, codes, defect)
        if defect == "wrong_level":
            rejects(R.assert_equal, r, res, defect)
    # a distance without dimension D - 1: on the census the winner's margin is in every digit, so plant the difference in the last one
    x, cb = R.rvq_near_tie_case(**R.NEAR_TIE)
    cb = cb.copy()
    near = E.rvq_level(x, cb)
    cb[near, -1] += 4.0                                            # the nearest entry is far in dimension D - 1 alone
    want = R.rvq_level_ref(x, cb)
    assert (want != near).any()
    rejects(R.assert_equal, R.rvq_level_ref(x, cb, defect="no_last_dim"), want)
    # ... and on the integer case with D = 1 the only dimension is the last
    s1, a1, c1, _ = R.rvq_int_case(3, 1, 4096, 2, seed=11)
    rejects(R.assert_equal, R.rvq_ref(s1, a1, c1, defect="no_last_dim")[1], R.rvq_ref(s1, a1, c1)[1])


def test_conv_comparisons_reject_a_leaking_start_and_a_zero_lo_plane():
    for K in (2, 7, 9):
        T, C = 12, 16
        pcm = g(7).integers(1, 5, T).astype(np.float32)            # pcm[0] != 0: the leak shows
        w, b = g(8).integers(-3, 4, (C, K)).astype(np.float32), g(9).integers(-3, 4, C).astype(np.float32)
        w[:, 0] = np.where(w[:, 0] == 0, 1, w[:, 0])
        good = R.conv0_ref(pcm, w, b, mirror=True)
        bad = R.conv0_ref(pcm, w, b, mirror=True, defect="leak")
        rejects(R.assert_equal, bad, good)
        R.assert_equal(bad[K - 1:], good[K - 1:])                   # only the first K - 1 outputs differ
    x = torch.from_numpy((3 * g(10).standard_normal((40, 16))).astype(np.float32))
    hi, lo, e64 = R.elu_planes_ref(x)
    hi0, lo0, _ = R.elu_planes_ref(x, defect="lo0")
    pos, neg = x >= 0, x < 0
    rejects(RR.check_bits, lo0[pos], lo[pos])
    rejects(RR.check_close, (hi0.float() + lo0.float())[neg], e64[neg], R.elu_neg_tol(e64)[neg])
    RR.check_close((hi.float() + lo.float())[neg], e64[neg], R.elu_neg_tol(e64)[neg])


def test_stats_comparisons_reject_a_variance_about_zero():
    for T, C in ((4, 5), (101, 65)):
        x = torch.from_numpy((1.5 + g(11).standard_normal((T, C))).astype(np.float32))
        ref, bad = R.stats_pool_ref(x), R.stats_pool_ref(x, defect="about_zero")
        _, ts = R.stats_pool_tol(x)
        RR.check_close(torch.from_numpy(R.stats_pool_mirror(x.numpy()))[C:], ref[C:], ts)
        rejects(RR.check_close, bad[C:], ref[C:], ts)
    # mean 1000, deviation 0.01: the two-pass mirror passes, a one-pass E[x^2] - mean^2 in float32 does not
    x = (1000.0 + 0.01 * g(12).standard_normal((101, 65))).astype(np.float32)
    ref = R.stats_pool_ref(x)
    _, ts = R.stats_pool_tol(x)
    RR.check_close(torch.from_numpy(R.stats_pool_mirror(x))[65:], ref[65:], ts)
    m = x.mean(0, dtype=np.float32)
    one_pass = np.sqrt(np.maximum((x * x).mean(0, dtype=np.float32) - m * m, 0) + np.float32(1e-5))
    rejects(RR.check_close, torch.from_numpy(one_pass), ref[65:], ts)
    assert R.ulps_apart(np.float32([1.0]), np.nextafter(np.float32([1.0]), np.float32(2)))[0] == 1


def test_gemv_comparisons_reject_a_dropped_last_row():
    for N, K in ((1, 1), (5, 65), (130, 63)):
        W, x, b = (g(13).standard_normal(n).astype(np.float32) for n in ((N, K), K, N))
        W[-1], b[-1] = np.abs(W[-1]) + 0.1, 0.5
        x = np.abs(x) + 0.1                                          # row N - 1 is positive: relu keeps it, zero is wrong
        for relu in (0, 1):
            y, mag = R.gemv_ref(W, b, x, relu)
            bad, _ = R.gemv_ref(W, b, x, relu, defect="no_last_row")
            RR.check_close((torch.from_numpy(W) @ torch.from_numpy(x) + torch.from_numpy(b)).clamp(min=0 if relu else -1e30), y, (K + 1) * R.U24 * mag)
            rejects(RR.check_close, bad, y, (K + 1) * R.U24 * mag)
    Wi, xi = g(14).integers(-4, 5, (5, 65)).astype(np.float32), g(15).integers(-4, 5, 65).astype(np.float32)
    Wi[-1], xi[:] = 1, np.abs(xi) + 1
    rejects(RR.check_bits, R.gemv_ref(Wi, None, xi, 0, defect="no_last_row")[0].float(), R.gemv_ref(Wi, None, xi, 0)[0].float())
