"""The four kernels of rho_tts_amd/csrc/encoder.hip one by one - k_enc_conv0, k_rvq<1..4>, k_stats_pool, k_gemv_f32 - through the
rt_debug_* hooks that call their production launchers, and the stages of the conditioning front-end through
rt_debug_voice_encode_stages, against tests/encoder_ref.py.

What is compared how:
* k_rvq: codes AND the returned residual EXACTLY (integers; float32 bit patterns), no tolerance, no frame left out - the hook feeds
  the reference's own vectors.  Every instantiation runs: K <= 1024 <1>, 1025 .. 2048 <2>, 2049 .. 3072 <3>, 3073 .. 4096 <4>.
* k_enc_conv0: x bit for bit against the float32 mirror of its evaluation order on both tap paths (taps <= 8 in registers, > 8 in a
  loop) and behind the grid-stride loop; hi / lo bit for bit where x >= 0, within elu_neg_tol (derived) where x < 0.
* k_stats_pool, k_gemv_f32: bit for bit on integer-valued operands, at bounds derived from the reduction length otherwise.
* stages: each against a float64 reference fed the GPU's own previous stage, at bounds derived layer by layer; the codes against
  rvq_ref of the GPU's own sem / aco, exactly.
Every output buffer has sentinel rows behind it that must come back untouched.  tests/test_encoder_ref_cpu.py shows that each of
these comparisons rejects a reference with one minimal defect, and that the near-tie input turns on the evaluation order."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import encoder_ref as R
from tests import rowops_ref as RR

pytestmark = pytest.mark.gpu

F64 = torch.float64
SENT = -77.0                         # exact in bf16 and float32; no output below equals it
ISENT = -77
PAD = 2                              # sentinel rows behind every output


@pytest.fixture(scope="module")
def ctx():
    from rho_tts_amd import _native
    c = _native.Context(0)
    yield c
    c.close()


def P(t):
    return None if t is None else t.data_ptr()


def dev(a):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a)).cuda()


def sent(*shape, dtype=torch.float32):
    return torch.full(shape, ISENT if dtype == torch.int32 else SENT, dtype=dtype, device="cuda")


def untouched(buf, rows, what):
    """the rows from `rows` on still hold the sentinel"""
    tail = buf[rows:].cpu()
    RR.check_bits(tail, torch.full_like(tail, ISENT if buf.dtype == torch.int32 else SENT), what + ": sentinel rows")


def refused(ctx, rc, what):
    assert rc != 0, f"{what}: launched instead of being refused"
    assert ctx.lib.rt_last_error(ctx.handle), what


def g(seed):
    return np.random.default_rng(seed)


# ================================================================================================ 1. k_rvq
def rvq(ctx, sem, aco, cbs, T=None, D=None, K=None, Q=None):
    """-> (rc, codes [T][Q] int64, aco after the call [T][D] float32); the sentinel rows are checked here.  T / D / K / Q override what
    the arrays say (the refusals)."""
    rows, width = sem.shape
    T, D, K, Q = (rows if T is None else T), (width if D is None else D), (cbs[0].shape[0] if K is None else K), (len(cbs) if Q is None else Q)
    d_sem = dev(sem)
    d_aco = sent(rows + PAD, width)
    d_aco[:rows] = dev(aco)
    d_codes = sent(rows + PAD, max(Q, 1), dtype=torch.int32)
    d_cb = [dev(cb.T) for cb in cbs]                              # transposed [D][K], as the kernel takes them
    arr = (C.c_void_p * len(d_cb))(*[t.data_ptr() for t in d_cb])
    torch.cuda.synchronize()
    rc = ctx.lib.rt_debug_rvq(ctx.handle, P(d_sem), P(d_aco), T, D, K, Q, arr, P(d_codes))
    untouched(d_codes, T if rc == 0 else 0, "codes")
    untouched(d_aco, rows, "aco")
    return rc, d_codes[:rows].cpu().numpy().astype(np.int64), d_aco[:rows].cpu().numpy()


def check_rvq(ctx, sem, aco, cbs, what):
    codes, res = R.rvq_ref(sem, aco, cbs)
    rc, got, got_res = rvq(ctx, sem, aco, cbs)
    ctx.check(rc, "rt_debug_rvq")
    R.assert_equal(got, codes, what + ": codes")
    R.assert_equal(got_res, res, what + (": aco is left alone (Q == 1)" if len(cbs) == 1 else ": residual after the last level"))
    return codes


# (T, D, K, Q): every K of the four instantiations and their edges, every D around the 8-dimension step and the 16-dimension double
# step (1, 7, 8, 9, 16, 17, 24, 40, 256), odd T (the last workgroup's second frame is a clamped duplicate that must write nothing)
RVQ_SHAPES = [(1, 1, 37, 1), (2, 7, 64, 2), (3, 8, 1000, 5), (33, 9, 1024, 2), (33, 16, 1025, 5), (3, 17, 2048, 1), (2, 24, 2049, 2),
              (33, 40, 3000, 5), (3, 256, 3073, 2), (33, 8, 4096, 5), (1, 17, 4096, 2), (3, 9, 37, 5), (2, 1, 4096, 1), (33, 256, 2048, 2)]


@pytest.mark.parametrize("T,D,K,Q", RVQ_SHAPES)
def test_rvq_integer_ties_and_normal_data(ctx, T, D, K, Q):
    """Integer form: distances are exact, duplicates of the winner are planted at two entries of one thread, two lanes of a wave, two
    waves, index 0, index K - 1 and in the last, partly filled wave (encoder_ref.rvq_tie_positions) - the index rule alone decides,
    in all three places it lives.  Normal form: plain float32 data, where the defined order decides."""
    sem, aco, cbs, _ = R.rvq_int_case(T, D, K, Q, seed=100 + K + D)
    check_rvq(ctx, sem, aco, cbs, f"int T={T} D={D} K={K} Q={Q}")
    r = g(200 + K + D)
    sem, aco = r.standard_normal((T, D)).astype(np.float32), r.standard_normal((T, D)).astype(np.float32)
    cbs = [(0.8 ** q * r.standard_normal((K, D))).astype(np.float32) for q in range(Q)]
    check_rvq(ctx, sem, aco, cbs, f"normal T={T} D={D} K={K} Q={Q}")


def test_rvq_at_the_lds_limit(ctx):
    """D = 4096: both frames' vectors fill 32 KiB of LDS; 256 double steps of the dimension loop."""
    T, D, K, Q = 3, 4096, 64, 2
    sem, aco, cbs, _ = R.rvq_int_case(T, D, K, Q, seed=7)
    check_rvq(ctx, sem, aco, cbs, "int D=4096")
    r = g(8)
    check_rvq(ctx, r.standard_normal((T, D)).astype(np.float32), r.standard_normal((T, D)).astype(np.float32),
              [r.standard_normal((K, D)).astype(np.float32) for _ in range(Q)], "normal D=4096")


@pytest.mark.parametrize("T,D,K,Q", [(33, 8, 3000, 5), (3, 1, 4096, 2), (2, 7, 1025, 5), (5, 40, 37, 2), (4, 4, 4096, 5), (3, 4096, 64, 2)])
def test_rvq_planted_census(ctx, T, D, K, Q):
    """x is entry target[t][q] of each level's codebook once the earlier levels are taken off: the codes must be the planted targets
    (frame 0 plants entry 0 at every level, the last frame entry K - 1) and nothing is left of aco."""
    sem, aco, cbs, target = R.rvq_census_case(T, D, K, Q, seed=12)
    codes = check_rvq(ctx, sem, aco, cbs, f"census T={T} D={D} K={K} Q={Q}")
    assert np.array_equal(codes, target)


@pytest.mark.parametrize("case", [R.NEAR_TIE, R.NEAR_TIE_2], ids=["K1100", "K2049"])
def test_rvq_near_ties_pin_the_evaluation_order(ctx, case):
    """The input on which a fused multiply-add, a descending sum and float64 distances each change codes
    (tests/test_encoder_ref_cpu.py asserts the counts): exact equality here says the kernel sums in the defined order.  The same
    vectors go to level 0 (as sem) and to level 1 (as aco)."""
    x, cb = R.rvq_near_tie_case(**case)
    check_rvq(ctx, x, x.copy(), [cb], "near tie, Q=1")
    check_rvq(ctx, x, x.copy(), [cb, cb.copy()], "near tie, Q=2")


def test_rvq_refusals_and_the_empty_call(ctx):
    r = g(9)
    sem, aco = r.standard_normal((3, 8)).astype(np.float32), r.standard_normal((3, 8)).astype(np.float32)
    big = [r.standard_normal((4097, 8)).astype(np.float32)] * 2
    rc, _, got = rvq(ctx, sem, aco, big)                                         # K = 4097
    refused(ctx, rc, "K=4097")
    R.assert_equal(got, aco)
    wide = r.standard_normal((2, 4097)).astype(np.float32)
    rc, _, got = rvq(ctx, wide, wide.copy(), [r.standard_normal((16, 4097)).astype(np.float32)] * 2)   # D = 4097
    refused(ctx, rc, "D=4097")
    R.assert_equal(got, wide)
    cbs = [r.standard_normal((64, 8)).astype(np.float32)] * 2
    rc, _, got = rvq(ctx, sem, aco, cbs, Q=0)
    refused(ctx, rc, "Q=0")
    R.assert_equal(got, aco)
    rc, _, got = rvq(ctx, sem, aco, cbs, T=0)                                    # nothing to do: OK, and nothing written
    ctx.check(rc, "rt_debug_rvq T=0")
    R.assert_equal(got, aco)


# ================================================================================================ 2. k_enc_conv0
def conv0(ctx, pcm, w, b, T=None, C_=None):
    rows, (Cw, K) = pcm.shape[0], w.shape
    T, C_ = (rows if T is None else T), (Cw if C_ is None else C_)
    x, hi, lo = sent(rows + PAD, Cw), sent(rows + PAD, Cw, dtype=torch.bfloat16), sent(rows + PAD, Cw, dtype=torch.bfloat16)
    keep = [dev(pcm if rows else np.zeros(1, np.float32)), dev(w), dev(b)]
    torch.cuda.synchronize()
    rc = ctx.lib.rt_debug_enc_conv0(ctx.handle, P(keep[0]), T, C_, K, P(keep[1]), P(keep[2]), P(x), P(hi), P(lo))
    n = T if rc == 0 else 0
    for buf, name in ((x, "x"), (hi, "hi"), (lo, "lo")):
        untouched(buf, n, name)
    return rc, x[:n].cpu(), hi[:n].cpu(), lo[:n].cpu()


def check_conv0(ctx, pcm, w, b, what):
    rc, x, hi, lo = conv0(ctx, pcm, w, b)
    ctx.check(rc, "rt_debug_enc_conv0")
    R.assert_equal(x.numpy(), R.conv0_ref(pcm, w, b, mirror=True), what + ": x against the float32 mirror")
    rhi, rlo, e64 = R.elu_planes_ref(x)                           # planes of the kernel's OWN x
    pos, neg = x >= 0, x < 0
    RR.check_bits(hi[pos], rhi[pos], what + ": hi where x >= 0")
    RR.check_bits(lo[pos], rlo[pos], what + ": lo where x >= 0")
    if bool(neg.any()):
        RR.check_close((hi.float() + lo.float())[neg], e64[neg], R.elu_neg_tol(e64)[neg], what + ": hi + lo where x < 0")
    return x


@pytest.mark.parametrize("taps", [1, 2, 7, 8, 9, 16])
@pytest.mark.parametrize("C_", [1, 16, 64, 256])
def test_enc_conv0(ctx, C_, taps):
    """taps <= 8: the register path (clamped, masked requests); 9 and 16: the loop.  T around the taps (outputs that are all causal
    zeros) and around 256 / C, the time steps of one workgroup, and 700 (several workgroups).  Integer form: x is exact, so the
    float64 reference rounded to float32 pins the causal zeros as well; random form: the mirror's bits."""
    per = 256 // C_
    for T in sorted({1, taps - 1, taps, per - 1, per, per + 1, 700} - {0}):
        r = g(1000 * C_ + 10 * taps + T)
        pcm, w, b = (r.integers(-4, 5, n).astype(np.float32) for n in (T, (C_, taps), C_))
        x = check_conv0(ctx, pcm, w, b, f"int C={C_} taps={taps} T={T}")
        R.assert_equal(x.numpy(), R.conv0_ref(pcm, w, b).astype(np.float32), "integer x against float64")
        pcm, w, b = (r.standard_normal(n).astype(np.float32) for n in (T, (C_, taps), C_))
        check_conv0(ctx, pcm, w, b, f"rand C={C_} taps={taps} T={T}")
    if taps == 1:                                                   # T = taps - 1 = 0: OK, nothing launched, nothing written
        rc, x, _, _ = conv0(ctx, np.zeros(0, np.float32), np.ones((C_, 1), np.float32), np.ones(C_, np.float32))
        ctx.check(rc, "rt_debug_enc_conv0 T=0")


def test_enc_conv0_grid_stride(ctx):
    """C = 64 and T = 4 x 65535 x 4 + 5: one more round of the grid-stride loop for the first five time steps of the grid.  Integer
    data, compared on the device against a broadcast reference (nothing is copied to the host but the verdicts)."""
    C_, T = 64, 4 * 65535 * 4 + 5
    gen = torch.Generator(device="cuda").manual_seed(5)
    pcm = torch.randint(-3, 4, (T,), generator=gen, device="cuda").float()
    w = torch.randint(-2, 3, (C_, 1), generator=gen, device="cuda").float()
    b = torch.randint(-2, 3, (C_,), generator=gen, device="cuda").float()
    x, hi, lo = sent(T + 1, C_), sent(T + 1, C_, dtype=torch.bfloat16), sent(T + 1, C_, dtype=torch.bfloat16)
    torch.cuda.synchronize()
    ctx.check(ctx.lib.rt_debug_enc_conv0(ctx.handle, P(pcm), T, C_, 1, P(w), P(b), P(x), P(hi), P(lo)), "rt_debug_enc_conv0")
    for buf in (x, hi, lo):
        assert bool((buf[T:] == SENT).all())
    ref = b[None, :] + w[:, 0][None, :] * pcm[:, None]            # |ref| <= 8: exact
    assert torch.equal(x[:T], ref)
    zero = torch.zeros((), device="cuda", dtype=torch.bfloat16)
    pos = ref >= 0                                                 # small integers: hi = x, lo = 0 there
    assert torch.equal(torch.where(pos, hi[:T], zero), torch.where(pos, ref.to(torch.bfloat16), zero))
    assert torch.equal(torch.where(pos, lo[:T], zero), torch.zeros_like(lo[:T]))
    e64 = torch.expm1(ref.to(F64))
    err = torch.where(pos, torch.zeros((), device="cuda", dtype=F64), (hi[:T].to(F64) + lo[:T].to(F64) - e64).abs() - R.elu_neg_tol(e64))
    assert float(err.max()) <= 0.0
    assert bool((~pos).any()) and bool(pos.any())


@pytest.mark.parametrize("C_", [48, 0, 512])
def test_enc_conv0_refuses_widths_that_do_not_divide_256(ctx, C_):
    pcm = np.ones(8, np.float32)
    w, b = np.ones((max(C_, 1), 7), np.float32), np.ones(max(C_, 1), np.float32)
    rc, _, _, _ = conv0(ctx, pcm, w, b, C_=C_)
    refused(ctx, rc, f"C={C_}")


# ================================================================================================ 3. k_stats_pool
def stats_pool(ctx, x, T=None):
    rows, C_ = x.shape
    out = sent(2 * C_ + PAD)
    keep = dev(x)
    torch.cuda.synchronize()
    rc = ctx.lib.rt_debug_stats_pool(ctx.handle, P(keep), rows if T is None else T, C_, P(out))
    untouched(out, 2 * C_ if rc == 0 else 0, "stats")
    return rc, out[:2 * C_].cpu()


@pytest.mark.parametrize("C_", [1, 63, 64, 65, 130])
def test_stats_pool(ctx, C_):
    """T = 1 .. 5 (fewer rows than time lanes, one lane with a second row) and 101; C across the 64-channel workgroup.
    Integer input: the sum is exact, so with T a power of two the mean is bit-exact and the deviation is the float32 mirror's to 2
    ulps (the division and the square root may each be off by one).  Every input: within stats_pool_tol, derived from T."""
    for T in (1, 2, 3, 4, 5, 101):
        r = g(100 * C_ + T)
        for form, x in (("int", r.integers(-8, 9, (T, C_)).astype(np.float32)), ("rand", (0.5 + r.standard_normal((T, C_))).astype(np.float32)),
                        ("offset", (1000.0 + 0.01 * r.standard_normal((T, C_))).astype(np.float32))):   # a one-pass variance would lose this one
            what = f"{form} T={T} C={C_}"
            rc, out = stats_pool(ctx, x)
            ctx.check(rc, "rt_debug_stats_pool")
            ref, (tm, ts) = R.stats_pool_ref(x), R.stats_pool_tol(x)
            em = RR.check_close(out[:C_], ref[:C_], tm, what + ": mean")
            es = RR.check_close(out[C_:], ref[C_:], ts, what + ": deviation")
            mir = R.stats_pool_mirror(x)
            ulps = int(R.ulps_apart(out[C_:].numpy(), mir[C_:]).max())
            print(f"stats_pool {what}: mean err {em:.2e} (bound {float(tm.max()):.2e}), deviation err {es:.2e} (bound {float(ts.max()):.2e}), {ulps} ulps from the mirror")
            if form == "int" and T in (1, 2, 4):
                RR.check_bits(out[:C_], ref[:C_].float(), what + ": mean of integers over a power of two")
                assert ulps <= 2, (what, ulps)
    rc, _ = stats_pool(ctx, np.zeros((1, C_), np.float32), T=0)
    refused(ctx, rc, "T=0")


# ================================================================================================ 4. k_gemv_f32
def gemv(ctx, W, b, x, relu):
    N, K = W.shape
    y = sent(N + PAD)
    keep = [dev(W), dev(b), dev(x)]
    torch.cuda.synchronize()
    rc = ctx.lib.rt_debug_gemv_f32(ctx.handle, P(keep[0]), P(keep[1]), P(keep[2]), N, K, relu, P(y))
    untouched(y, N, "y")
    return rc, y[:N].cpu()


@pytest.mark.parametrize("N", [1, 3, 4, 5, 130])
def test_gemv_f32(ctx, N):
    """N across the four rows of a workgroup, K across the 64 lanes of a row's wave; bias present and NULL, relu on and off; the
    sums fall on both sides of zero (asserted).  Integer operands: every partial sum is an integer, bit for bit.  Random operands:
    (K + 1) u sum |w||x|, the bias counted as one more term of the sum (encoder_ref.gemv_ref)."""
    for K in (1, 63, 64, 65, 1000):
        r = g(1000 * N + K)
        Wi, xi, bi = (r.integers(-4, 5, n).astype(np.float32) for n in ((N, K), K, N))
        Wr, xr, br = (r.standard_normal(n).astype(np.float32) for n in ((N, K), K, N))
        if N >= 2:                                                  # both signs, whatever the draw: row 0 positive, row 1 negative
            for W_, x_ in ((Wi, xi), (Wr, xr)):
                x_[x_ == 0] = 1
                W_[0], W_[1] = np.abs(W_[0]) * np.sign(x_) + np.sign(x_), -(np.abs(W_[1]) * np.sign(x_) + np.sign(x_))
        for use_b in (False, True):
            for relu in (0, 1):
                what = f"N={N} K={K} bias={use_b} relu={relu}"
                ref, _ = R.gemv_ref(Wi, bi if use_b else None, xi, relu)
                rc, y = gemv(ctx, Wi, bi if use_b else None, xi, relu)
                ctx.check(rc, "rt_debug_gemv_f32")
                RR.check_bits(y, ref.float(), "int " + what)
                ref, mag = R.gemv_ref(Wr, br if use_b else None, xr, relu)
                rc, y = gemv(ctx, Wr, br if use_b else None, xr, relu)
                ctx.check(rc, "rt_debug_gemv_f32")
                RR.check_close(y, ref, (K + 1) * R.U24 * mag, "rand " + what)
                if N >= 2 and not use_b:
                    pre, _ = R.gemv_ref(Wr, None, xr, 0)
                    assert float(pre[0]) > 0 > float(pre[1])
                    assert not relu or float(y[1]) == 0.0


# ================================================================================================ 5. the stages of voice_encode_impl
def encode_stages(nm, cfg, pcm):
    c = cfg.codec
    F_ = pcm.size // c.total_upsample
    He, Dq, Q = c.enc_hidden, c.vq_dim, c.num_quantizers
    f32 = np.float32
    out = dict(feats=np.full((2 * F_, He), SENT, f32), tf=np.full((2 * F_, He), SENT, f32), emb=np.full((F_, He), SENT, f32),
               sem=np.full((F_, Dq), SENT, f32), aco=np.full((F_, Dq), SENT, f32))
    codes = np.full((F_, Q), ISENT, np.int32)
    spk = np.zeros(cfg.talker.hidden, f32)
    nf = C.c_int32()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = nm.lib.rt_debug_voice_encode_stages(nm.handle, pcm.ctypes.data_as(C.POINTER(C.c_float)), pcm.size, F_, vp(out["feats"]), vp(out["tf"]),
                                             vp(out["emb"]), vp(out["sem"]), vp(out["aco"]), codes.ctypes.data_as(C.POINTER(C.c_int32)),
                                             C.byref(nf), vp(spk))
    nm.ctx.check(rc, "rt_debug_voice_encode_stages")
    assert nf.value == F_
    return out, codes.astype(np.int64), spk


@pytest.mark.parametrize("preset,n_frames", [("tiny", 37), ("small", 50)])
def test_encoder_stages(ctx, preset, n_frames):
    """Each stage against a float64 reference FED THE GPU'S OWN PREVIOUS STAGE, so errors do not compound: feats against the conv
    encoder chained in float64 on the clip (first-order bound through the chain's own Jacobian: encoder_ref.seanet_ref), emb
    against the float64 down-sampling conv of the GPU's tf, sem / aco against the float64 projections of the GPU's emb
    (encoder_ref._conv_bounded: 16 operand bits and 2 K + 2 float32 roundings), and the codes against rvq_ref of the GPU's own
    sem / aco EXACTLY - which is what makes "the argmin equals the oracle's bit for bit" true on the real pipeline.  The CPU
    float32 oracle's own error against the same float64 references is printed next to the GPU's (DESIGN.md records both)."""
    from oracle import encoder as E
    from rho_tts_amd import config
    from tests.test_encoder_gpu import build, clip
    cfg = config.PRESETS[preset]()
    nm, W = build(ctx, cfg)
    try:
        pcm = clip(cfg, n_frames, 1)
        got, codes, spk = encode_stages(nm, cfg, pcm)
        codes_pub, spk_pub = nm.encode_voice(pcm)                   # the public entry point launches the same: the same answer
        assert np.array_equal(codes_pub.numpy(), codes) and np.allclose(spk_pub.numpy(), spk, rtol=0, atol=1e-6 * float(np.abs(spk).max()))
        _, _, mid = E.encode(W, cfg, pcm, return_intermediates=True)
        T = lambda a: torch.from_numpy(a)
        rel = lambda e, ref: float(e) / float(ref.abs().max())

        feats, bound = R.seanet_ref(W, cfg, pcm)
        assert bool(np.isfinite(got["feats"]).all())
        err = (T(got["feats"]).to(F64) - feats).abs().reshape(-1)
        idx = R.feats_check_indices(err, feats.shape)               # first row, last row, the 32 largest errors: a Jacobian row each
        fb = bound(idx)
        over = err[idx] > fb
        assert not bool(over.any()), f"feats: {int(over.sum())} elements over their bound, worst {float((err[idx] / fb).max()):.2f} x"
        assert float(err.max()) <= float(fb.max())                  # (everything else: under the largest bound derived)
        print(f"\n{preset} feats: GPU {rel(err.max(), feats):.2e}, CPU float32 {rel((mid['feats'].to(F64) - feats).abs().max(), feats):.2e}, "
              f"bound {rel(fb.min(), feats):.2e} .. {rel(fb.max(), feats):.2e} (of max |feats|), largest error / bound {float((err[idx] / fb).max()):.3f}")

        emb, eb = R.downsample_ref(W, got["tf"])
        e_gpu = RR.check_close(T(got["emb"]), emb, eb, "emb")
        cpu = E.causal_conv(T(got["tf"]).T[None], W["enc.downsample.weight"], None, stride=2, pad_mode="replicate")[0].T
        print(f"{preset} emb: GPU {rel(e_gpu, emb):.2e}, CPU float32 {rel((cpu.to(F64) - emb).abs().max(), emb):.2e}, bound {rel(eb.max(), emb):.2e}")

        for name, which in (("sem", "semantic"), ("aco", "acoustic")):
            ref, rb = R.projection_ref(W, got["emb"], which)
            e_gpu = RR.check_close(T(got[name]), ref, rb, name)
            cpu = T(got["emb"]) @ W[f"enc.vq.{which}.input_proj.weight"].T
            print(f"{preset} {name}: GPU {rel(e_gpu, ref):.2e}, CPU float32 {rel((cpu.to(F64) - ref).abs().max(), ref):.2e}, bound {rel(rb.max(), ref):.2e}")

        cbs = [W[f"enc.vq.codebook.{q}"].numpy() for q in range(cfg.codec.num_quantizers)]
        want, _ = R.rvq_ref(got["sem"], got["aco"], cbs)
        R.assert_equal(codes, want, "codes against rvq_ref of the GPU's own sem / aco")
    finally:
        nm.close()


# ================================================================================================ 6. non-finite audio
@pytest.mark.parametrize("bad", [float("nan"), float("inf")], ids=["nan", "inf"])
def test_non_finite_audio_is_refused_before_the_gpu(ctx, bad):
    """One NaN or infinite sample: encode_voice and set_voice_pcm raise ValueError naming the sample (the host check of
    voice_encode_impl, before anything is launched), the installed voice stays, and the model generates as before."""
    from rho_tts_amd import config
    from rho_tts_amd._native_model import RtSampling
    from tests.test_encoder_gpu import build, clip
    cfg = config.tiny()
    nm, _ = build(ctx, cfg)
    try:
        pcm = clip(cfg, 21, 2)
        sp = RtSampling(1, 0.9, 50, 1.0, 1.05)
        n_rows, codes = nm.set_voice_pcm(pcm, "english", [5, 6, 7, 8])
        a = nm.generate([[10, 11, 12], [20, 21]], [6, 5], sp, seed=3)
        x = pcm.copy()
        x[pcm.size // 2] = bad
        with pytest.raises(ValueError, match=f"sample {pcm.size // 2} "):
            nm.encode_voice(x)
        with pytest.raises(ValueError, match=f"sample {pcm.size // 2} "):
            nm.set_voice_pcm(x, "english", [5, 6, 7, 8])
        assert nm.prefix_len() == n_rows
        b = nm.generate([[10, 11, 12], [20, 21]], [6, 5], sp, seed=3)
        assert all(torch.equal(p, q) for p, q in zip(a, b))
        c2, _ = nm.encode_voice(pcm)
        assert torch.equal(c2, codes)
        tail = np.concatenate([pcm, np.float32([bad, 0.0])])       # behind the last whole frame a sample is never uploaded, never read
        c3, _ = nm.encode_voice(tail)
        assert torch.equal(c3, codes)
    finally:
        nm.close()
