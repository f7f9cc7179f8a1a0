"""The two launch-plan switches of the decode GEMM's prologue, bit for bit against the launches they replace:

3400/3401  rows of n RMSNorm sum-of-squares partials (n % 64 == 0, n <= 256) stored plainly and fetched one dword per request /
           stored permuted (csrc/common.h rowsq_slot) and fetched in 16-byte requests by the row-scale prologue
3500/3501  STORE / RESID launches of up to 32 rows: weight / activation chunks of 8 k-tiles / of the length of the wave's run

Neither changes which values a lane adds nor in which order, so every comparison between the two values of a switch is torch.equal.
The RESID check also pins the Python mirror of rowsq_slot (tests/test_rowsq_layout_cpu.py) to the native function."""
import dataclasses

import pytest
import torch

from rho_tts_amd import config
from rho_tts_amd.config import TransformerDims
from tests.test_gemm_col_gpu import RESID, SILU, STORE, run_col
from tests.test_model_gpu import build, make_voice, set_voice
from tests.test_rowsq_layout_cpu import rowsq_slot

pytestmark = pytest.mark.gpu

ROWS = [1, 15, 16, 17, 32, 33, 64, 65, 128]
SAMPLED = (1, 0.9, 50, 1.0, 1.05)


@pytest.fixture(scope="module")
def ctx():
    from rho_tts_amd import _native
    c = _native.Context(0)
    yield c
    c.close()


def wide_off_then_on(lib, run):
    """run() with plain rows and narrow requests (3400), then with the default that is left behind (3401)"""
    try:
        lib.rt_debug_tune(3400, 0)
        off = run()
    finally:
        lib.rt_debug_tune(3401, 0)
    return off, run()


def fit_off_then_on(lib, run):
    try:
        lib.rt_debug_tune(3500, 0)
        off = run()
    finally:
        lib.rt_debug_tune(3501, 0)
    return off, run()


def operands(M, N, K, seed):
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(M, K, generator=g).to(torch.bfloat16).cuda()
    w = (torch.randn(N, K, generator=g) * 0.05).to(torch.bfloat16).cuda()
    return g, a, w


def slots(n):
    return torch.tensor([rowsq_slot(j, n) for j in range(n)], device="cuda")


# ------------------------------------------------------------------------------------------------ the producer: RESID's partials
@pytest.mark.parametrize("N", [512, 1024, 2048])
@pytest.mark.parametrize("split", [1, 2])
def test_resid_stores_each_partial_at_its_slot(ctx, N, split):
    """n_part = N / 16 * split is 32 (N = 512 unsplit: the identity), 64, 128 or 256.  Partial j of a row - the sum of squares of
    the 16 / split columns of the new x that workgroup j owns - must stand at rowsq_slot(j, n_part); x, the next operand and the
    partials as a multiset must not depend on the layout.  The partial itself: 16 / split exact-to-rounding squares added in f32,
    at most 5 roundings of 2^-24 each on a sum of non-negative terms, against float64 at 1e-6."""
    K, n_part, cw = 256, N // 16 * split, 16 // split
    perm = slots(n_part)
    for M in ROWS:
        g, a, w = operands(M, N, K, 100 + M)
        x0 = torch.randn(M, N, generator=g).cuda()
        scale = (0.5 + torch.rand(N, generator=g)).cuda()
        nw = (1.0 + 0.1 * torch.randn(N, generator=g)).cuda()
        for row_off in (0, 32):
            off, on = wide_off_then_on(ctx.lib, lambda: run_col(ctx, a, w, RESID, split, row_off, 1, None, 1e-6, None, scale, x0, nw))
            assert torch.equal(off["out"], on["out"]) and torch.equal(off["next"], on["next"]), (M, row_off)
            p_off, p_on = off["rowsq_out"][: M * n_part].view(M, n_part), on["rowsq_out"][: M * n_part].view(M, n_part)
            assert torch.equal(p_on[:, perm], p_off), (M, row_off)                       # partial j at slot(j): the native function is the mirror
            assert torch.equal(p_on.sort(1).values, p_off.sort(1).values)
            want = (on["out"].double() ** 2).view(M, n_part, cw).sum(2)
            assert float(((p_off.double() - want).abs() / want).max()) < 1e-6, (M, row_off)
    if n_part % 64:
        assert torch.equal(perm, torch.arange(n_part, device="cuda"))


# ------------------------------------------------------------------------------------------------ the consumers: the NORM prologue
@pytest.mark.parametrize("n", [64, 128, 256, 24])
@pytest.mark.parametrize("epi", [STORE, SILU])
def test_norm_consumers_read_the_permuted_rows(ctx, epi, n):
    """Distinct random partials, laid out plainly for 3400 and through rowsq_slot for 3401 (n = 24: no permutation, the narrow form
    both times).  n = 64 clamps the second of two 16-byte requests, n = 128 needs both, n = 256 takes the four-request form.
    The row scale itself (STORE: scaled over unscaled output, where that is at least a tenth of the largest) against float64:
    a sum of n <= 256 positive f32 terms, the hardware rsqrt and two output roundings - 1e-5 relative, which a dropped partial
    (1 / 256 of the sum: 2e-3 of the scale) misses by two orders of magnitude."""
    N, K = 64, 256
    perm = slots(n)
    for M in ROWS:
        g, a, w = operands(M, N, K, 200 + M)
        parts = (0.5 + torch.rand(M, n, generator=g)).cuda() * (K / n)
        permuted = torch.empty_like(parts)
        permuted[:, perm] = parts
        key = "out" if epi == STORE else "act"
        for row_off in (0, 32):
            try:
                ctx.lib.rt_debug_tune(3400, 0)
                off = run_col(ctx, a, w, epi, 0, row_off, 1, parts, 1e-6)[key]
            finally:
                ctx.lib.rt_debug_tune(3401, 0)
            on = run_col(ctx, a, w, epi, 0, row_off, 1, permuted, 1e-6)[key]
            assert torch.equal(off, on), (M, row_off)
            if epi == STORE:        # the row scale alone: the scaled output over the unscaled one, where that is not small
                plain = run_col(ctx, a, w, epi, 0, row_off, 1, None, 1e-6)[key].double()
                want = torch.rsqrt(parts.double().sum(1) / K + 1e-6)[:, None].expand_as(plain)
                big = plain.abs() > 0.1 * float(plain.abs().max())
                assert float(((on.double() / plain - want).abs() / want)[big].max()) < 1e-5, (M, row_off)


# ------------------------------------------------------------------------------------------------ fitted chunks
@pytest.mark.parametrize("K", [224, 256, 1024, 2048, 3072])
@pytest.mark.parametrize("M", [1, 32])
def test_fitted_chunks_change_no_bit(ctx, K, M):
    """A wave's run is K / 256 k-tiles: 1 (K = 224: seven k-tiles for eight waves, the guarded form; 256), 4 (1024: one chunk of 4),
    8 (2048: chunks of 8 either way) or 12 (3072: two chunks of 6 against 8 + 4 and four clamped re-loads).  Same k order inside a
    wave, so all three epilogues equal the chunks of 8 (3500) bit for bit."""
    N = 64
    g, a, w = operands(M, N, K, 300 + K + M)
    x0 = torch.randn(M, N, generator=g).cuda()
    scale = (0.5 + torch.rand(N, generator=g)).cuda()
    nw = (1.0 + 0.1 * torch.randn(N, generator=g)).cuda()
    bias = torch.randn(N, generator=g).cuda()
    parts = (0.5 + torch.rand(M, 128, generator=g)).cuda() * (K / 128)

    def run():
        return (run_col(ctx, a, w, STORE, 0, 0, 1, None, 1e-6, bias)["out"], run_col(ctx, a, w, STORE, 0, 0, 1, parts, 1e-6, bias)["out"],
                run_col(ctx, a, w, SILU, 0, 0, 1, parts, 1e-6)["act"], run_col(ctx, a, w, RESID, 2, 0, 1, None, 1e-6, None, scale, x0, nw))
    off, on = fit_off_then_on(ctx.lib, run)
    for i in range(3):
        assert torch.equal(off[i], on[i]), i
    for key in ("out", "next", "rowsq_out"):
        assert torch.equal(off[3][key], on[3][key]), key
    ref = a.double() @ w.double().T + bias.double()
    assert float((on[0].double() - ref).abs().max()) < 2e-3 * float(ref.abs().max())


# ------------------------------------------------------------------------------------------------ end to end
def equal_width(base):
    """talker and predictor both 512 wide: 64 partials per row in both stacks, no mtp projection (k_norm_tiled_rows reads the talker's rows)"""
    return dataclasses.replace(base, name="small-equal-512", predictor=TransformerDims(hidden=512, layers=2, heads=4, kv_heads=2, head_dim=128, inter=512))


def ragged(cfg, n, seed, lo=3, hi=9):
    g = torch.Generator().manual_seed(seed)
    texts = [[int(v) for v in torch.randint(0, cfg.text_vocab - 64, (int(k),), generator=g)] for k in torch.randint(1, 9, (n,), generator=g)]
    frames = [int(v) for v in torch.randint(lo, hi, (n,), generator=g)]
    return texts, frames


@pytest.mark.parametrize("which", ["small", "small-equal-512"])
def test_generation_is_the_same_with_either_layout(ctx, which):
    """small: the talker (hidden 512, split in half tiles) has 64 partials per row - the wide form - and the predictor (hidden 256)
    32, the narrow one.  16 ragged items on 16 rows with sampling: codes and both logit traces; then 13 items on 4 rows (rows handed
    over between frames)."""
    from rho_tts_amd._native_model import RtSampling
    cfg = config.PRESETS["small"]()
    if which != "small":
        cfg = equal_width(cfg)
        assert not cfg.has_mtp_proj
    assert ctx.device_info()["n_cu"] >= 64          # (hidden 512 is split in half tiles: 64 partials)
    nm, _ = build(ctx, cfg, max_batch=16)
    try:
        set_voice(nm, make_voice(cfg, True))
        texts, frames = ragged(cfg, 16, 3)
        for pair in (wide_off_then_on, fit_off_then_on):
            (codes_off, tr_off), (codes_on, tr_on) = pair(nm.lib, lambda: nm.generate(texts, frames, RtSampling(*SAMPLED), seed=77, trace=True))
            assert all(torch.equal(a, b) for a, b in zip(codes_off, codes_on))
            assert torch.equal(tr_off["talker"], tr_on["talker"]) and torch.equal(tr_off["predictor"], tr_on["predictor"])
            assert len({tuple(c.flatten().tolist()) for c in codes_on}) > 1
    finally:
        nm.close()
    nm, _ = build(ctx, cfg, max_batch=4)
    try:
        set_voice(nm, make_voice(cfg, True))
        texts, frames = ragged(cfg, 13, 17, 3, 12)
        ids = [100 + 7 * i for i in range(13)]

        def run():
            return nm.generate(texts, frames, RtSampling(*SAMPLED), seed=5, item_ids=ids), nm.generate_stats()
        (off, st_off), (on, st_on) = wide_off_then_on(nm.lib, run)
        assert st_on["rows"] == 4 and st_on["hand_overs"] >= 2 and st_on == st_off
        assert [c.shape[0] for c in on] == frames and all(torch.equal(a, b) for a, b in zip(off, on))
    finally:
        nm.close()
