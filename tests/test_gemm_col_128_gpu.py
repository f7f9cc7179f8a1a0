"""The 128-row instantiation of the column-owner decode GEMM (gemm_col.hip k_gemm_col, MT = 8) through rt_debug_gemm_col.

The property is bit identity with the launches that existed before it: a row of a 65..128-row launch must get exactly what
the 64-row launches (MT = 4 / 2 / 1 at the matching row offset) give it - the same 8-wave K split, the same k order in a wave,
the same order in the LDS combine.  So every comparison is torch.equal.

Rows: each sub-block edge above 64 (65, 80, 81, 96, 113), the ragged last row (127) and the full 128.
K = 32 is one k-tile for eight waves (the guarded NPRE = 0 form), K = 224 seven k-tiles (fewer than waves), K = 2048 two
super-chunks per wave.  N = 48 is three tiles (sub-tile split 2), N = 1024 many; gate/up of N = 12288 takes the
1.5-pairs-per-workgroup form on a 256-CU device (K = 32 / 224 only: it is there for the form, not for the depth).
The RESID and SILU epilogues write FRAGMENT-TILED outputs (the residual stream, the activations), whose layout exists for
widths that are multiples of 32 only (tile_off; rt_generate demands it of every model): at an output width of 48 the tiles
of neighbouring row blocks overlap and workgroups race for them, on any launch form.  So the narrow case of those two is
the nearest width the layout has: N = 96 for RESID, N = 192 (96 activations) for SILU; STORE is row-major and keeps N = 48.
"""
import numpy as np
import pytest
import torch

from tests.test_gemm_col_gpu import RESID, SILU, STORE, ints, run_col, used_split

pytestmark = pytest.mark.gpu

ROWS = [65, 80, 81, 96, 113, 127, 128]
DEPTHS = [32, 224, 2048]
# (epi, N, with RMSNorm row scale)
FORMS = [(STORE, 48, False), (STORE, 48, True), (STORE, 1024, False), (STORE, 1024, True), (RESID, 96, False), (RESID, 1024, False),
         (SILU, 192, True), (SILU, 1024, True), (SILU, 12288, True)]
KEYS = ("out", "next", "rowsq_out", "act")


@pytest.fixture(scope="module")
def ctx():
    from rho_tts_amd import _native
    c = _native.Context(0)
    yield c
    c.lib.rt_debug_tune(3201, 0)
    c.close()


def forms_for(K):
    return [f for f in FORMS if f[1] != 12288 or K <= 224]


def operands(M, K, N, epi, norm, seed):
    """Random bf16 operands as a decode step has them (cached per shape: the reference launches reuse them)."""
    g = torch.Generator().manual_seed(seed)
    x_prev = torch.randn(M, K, generator=g)
    a = ((1.0 + 0.1 * torch.randn(K, generator=g)) * x_prev).to(torch.bfloat16).cuda()
    w = (torch.randn(N, K, generator=g) * 0.05).to(torch.bfloat16).cuda()
    parts = 8 if K % 8 == 0 and K >= 64 else 1
    kw = dict(rowsq=(x_prev ** 2).view(M, parts, K // parts).sum(2).cuda() if norm else None)
    if epi == STORE:
        kw["bias"] = (torch.randn(N, generator=g) * 0.1).cuda()
    elif epi == RESID:
        kw.update(scale=(0.5 + torch.rand(N, generator=g)).cuda(), x=torch.randn(M, N, generator=g).cuda(),
                  next_w=(1.0 + 0.1 * torch.randn(N, generator=g)).cuda())
    return a, w, kw


def call(ctx, a, w, epi, row_off, kw, lo=0, hi=None):
    """rt_debug_gemm_col on rows [lo, hi) of the operands, placed at row_off + lo."""
    hi = a.shape[0] if hi is None else hi
    sl = lambda t: None if t is None else t[lo:hi].contiguous()
    return run_col(ctx, a[lo:hi].contiguous(), w, epi, 0, row_off + lo, 1, sl(kw.get("rowsq")), 1e-6, kw.get("bias"), kw.get("scale"),
                   sl(kw.get("x")), kw.get("next_w"))


def written(ctx, res, M, N):
    """The tensors a launch produced, cut to what it writes (rowsq_out: M x (tiles x split) partials)."""
    out = {}
    for k in KEYS:
        t = res[k]
        if t is None:
            continue
        out[k] = t[: M * ((N + 15) // 16) * used_split(ctx, N, 0)] if k == "rowsq_out" else t
    return out


def by_64(ctx, a, w, epi, row_off, kw, N):
    """The same rows from launches of <= 64 rows at the matching row offsets: the path that existed before MT = 8."""
    M = a.shape[0]
    lo, hi = written(ctx, call(ctx, a, w, epi, row_off, kw, 0, 64), 64, N), written(ctx, call(ctx, a, w, epi, row_off, kw, 64, M), M - 64, N)
    return {k: torch.cat([lo[k], hi[k]]) for k in lo}


@pytest.mark.parametrize("K", DEPTHS)
@pytest.mark.parametrize("M", ROWS)
def test_rows_equal_the_64_row_launches_bit_for_bit(ctx, M, K):
    """Checks 1 and 2: one 128-row launch (rt_debug_tune 3201) == launches of <= 64 rows == the same call under 3200."""
    for epi, N, norm in forms_for(K):
        a, w, kw = operands(M, K, N, epi, norm, 1000 * epi + N + K)
        for row_off in (0, 16):
            ctx.lib.rt_debug_tune(3201, 0)
            one = written(ctx, call(ctx, a, w, epi, row_off, kw), M, N)
            ref = by_64(ctx, a, w, epi, row_off, kw, N)
            ctx.lib.rt_debug_tune(3200, 0)
            two = written(ctx, call(ctx, a, w, epi, row_off, kw), M, N)
            ctx.lib.rt_debug_tune(3201, 0)
            assert set(one) == set(ref) == set(two) and one
            for k in one:
                assert not bool(torch.isnan(one[k].float()).any()), (epi, N, norm, row_off, k)
                assert torch.equal(one[k], ref[k]), (epi, N, norm, row_off, k, "128-row launch against <= 64-row launches")
                assert torch.equal(one[k], two[k]), (epi, N, norm, row_off, k, "3201 against 3200")
            main = one["act" if epi == SILU else "out"].float()
            assert float(main.abs().max()) > 1e-3                          # (the comparison is not one of zeros)


@pytest.mark.parametrize("K", DEPTHS)
@pytest.mark.parametrize("M", ROWS)
def test_small_integer_operands_are_exact(ctx, M, K):
    """Check 3: |a|, |w| <= 4 - every product and partial sum is an integer below 2^24, so STORE and RESID must equal the exact
    numpy product whatever the summation order.  (Under the SwiGLU only the integers are exact: expf and the bf16 rounding of
    the product remain, bounded as tests/test_gemm_col_gpu.py bounds them; its bits are pinned by the test above.)"""
    a = ints((M, K), -4, 4, 3 + M)
    for epi, N, _ in forms_for(K):
        w = ints((N, K), -4, 4, 5 + N)
        ref = torch.from_numpy(a.float().numpy().astype(np.float64) @ w.float().numpy().astype(np.float64).T)
        assert float(ref.abs().max()) < 2 ** 24
        ref = ref.float().cuda()
        for row_off in (0, 16):
            if epi == STORE:
                bias = ints((N,), -8, 8, 7).float().cuda()
                got = call(ctx, a.cuda(), w.cuda(), STORE, row_off, dict(bias=bias))["out"]
                assert torch.equal(got, ref + bias), (N, row_off)
            elif epi == RESID:
                x0 = ints((M, N), -16, 16, 9).float().cuda()
                kw = dict(scale=torch.full((N,), 0.25, device="cuda"), x=x0, next_w=torch.full((N,), 2.0, device="cuda"))
                r = call(ctx, a.cuda(), w.cuda(), RESID, row_off, kw)
                want = x0 + 0.25 * ref
                assert torch.equal(r["out"], want), (N, row_off)
                assert torch.equal(r["next"].float(), (2.0 * want).to(torch.bfloat16).float())
                n_part = (N + 15) // 16 * used_split(ctx, N, 0)
                # (the sums of squares pass 2^24: float32 rounding of each 16-column partial, as in tests/test_gemm_col_gpu.py)
                rq, want_sq = r["rowsq_out"][: M * n_part].view(M, n_part).double().sum(1), (want.double() ** 2).sum(1)
                assert float(((rq - want_sq).abs() / want_sq.clamp(min=1)).max()) < 1e-5, (N, row_off)
            else:
                got = call(ctx, a.cuda(), w.cuda(), SILU, row_off, {})["act"].float()
                g, u = ref[:, : N // 2], ref[:, N // 2:]
                want = torch.nn.functional.silu(g) * u
                assert float(((got - want).abs() / want.abs().clamp(min=1.0)).max()) <= 2.0 ** -7, (N, row_off)
                assert bool((got[(g == 0) | (u == 0)] == 0).all())


def test_more_than_128_rows_are_refused(ctx):
    a, w, kw = operands(129, 32, 48, STORE, False, 1)
    with pytest.raises(Exception):
        call(ctx, a, w, STORE, 0, kw)
