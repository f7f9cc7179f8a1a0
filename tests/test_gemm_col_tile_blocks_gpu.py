"""Tile blocks of the column-owner decode GEMM (gemm_col.hip k_gemm_col, RB + HP; rt_debug_tune 3700 / 3701 / 3702) through rt_debug_gemm_col.

A STORE / RESID launch at split 2 whose half-tile workgroups fill more than half of the CUs (on 256 CUs: N in 1040..2048, the 1.7B
talker's o / down and the predictor's head) runs whole-tile workgroups with its rows dealt over gridDim.y: 33..64 rows as two 32-row
blocks (3701), 17..32 rows as two 16-row blocks as well (3702).  Every column keeps its 8-wave K split, its k order inside a wave and
the ww = 0..7 order of the combine, and a whole-tile RESID workgroup stores the two half-tile sums of squares that the two half-tile
workgroups store (the rowsq row keeps its split-2 layout), so every output must equal the half-tile launch (3700) BIT FOR BIT - every
comparison here is torch.equal on out, next and rowsq_out.

Shapes follow the device's CU count.  N: both ends of the window and a middle whose 2 x tiles partials are no multiple of 64 (plain
rowsq rows; 256 partials at the upper end are permuted rows) - 1040, 1552, 2048 on 256 CUs.  K = 32 is one k-tile for eight waves (the
guarded NPRE = 0 form), 224 fewer k-tiles than waves, 1024 a run of 4 (one fitted chunk), 3072 a run of 12 (two chunks of 6), 6144 a
run of 24 (three chunks of 8).  Rows: each block edge and the ragged ends of both block sizes; 16 and 65 rows take no blocks.
rt_debug_col_tile_blocks - the launcher's rule as host arithmetic - says for every case which form it took, so that no comparison is
one of a launch with itself.
"""
import dataclasses
import os
import re

import numpy as np
import pytest
import torch

from tests.test_gemm_col_gpu import RESID, STORE, ints, run_col

pytestmark = pytest.mark.gpu

ROWS = [17, 24, 31, 32, 33, 47, 48, 49, 63, 64]
DEPTHS = [32, 224, 1024, 3072, 6144]
# (epi, partials per rowsq row of the RMSNorm row scale; 0 = none)
FORMS = [(RESID, 0), (STORE, 0), (STORE, 128)]
KEYS = ("out", "next", "rowsq_out")


def shipped(base, name):
    """The shipped value of a switch, from the one table of them."""
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rho_tts_amd", "csrc", "knobs.h")).read()
    return int(re.search(r"X\(%d, %s, (\d+)," % (base, name), src).group(1))


@pytest.fixture(scope="module")
def ctx():
    from rho_tts_amd import _native
    c = _native.Context(0)
    yield c
    switch(c, 3700 + shipped(3700, "g_col_tile_blocks"))
    c.close()


def switch(ctx, code):
    assert ctx.lib.rt_debug_tune(code, 0) == 0, code


_device = {}


def n_cu(ctx):
    if "n_cu" not in _device:
        _device["n_cu"] = ctx.device_info()["n_cu"]
    return _device["n_cu"]


def widths(ctx):
    """The window's ends and a middle with an odd tile count: split 2 fits the CUs (tiles <= n_cu / 2) and fills more than half of them."""
    lo, hi = n_cu(ctx) // 4 + 1, n_cu(ctx) // 2
    return [16 * lo, 16 * (((lo + hi) // 2) | 1), 16 * hi]


def tile_rows(ctx, M, N, epi):
    """Rows per block of such a launch under the current switches (0: the launch keeps its half-tile workgroups)."""
    return ctx.lib.rt_debug_col_tile_blocks(n_cu(ctx), M, N, epi, 0)


def expected_block(M, value):
    return 32 if (value >= 1 and 33 <= M <= 64) else 16 if (value >= 2 and 17 <= M <= 32) else 0


_weights, _acts = {}, {}


def operands(M, K, N, epi, parts):
    """Random bf16 operands as a decode step has them; the weight matrix is made once per (N, K), the rest once per case, and every
    launch that is compared reads the same tensors."""
    if (N, K) not in _weights:
        _weights.clear()        # (one matrix at a time)
        _weights[(N, K)] = (torch.randn(N, K, generator=torch.Generator().manual_seed(N + K)) * 0.05).to(torch.bfloat16).cuda()
    key = (M, K, N, epi, parts)
    if key not in _acts:
        g = torch.Generator().manual_seed(1000 * epi + N + K + 7 * M + parts)
        x_prev = torch.randn(M, K, generator=g)
        a = ((1.0 + 0.1 * torch.randn(K, generator=g)) * x_prev).to(torch.bfloat16).cuda()
        kw = {}
        if parts:           # partial sums of squares whose total is the row's: a row scale of the usual size
            share = torch.rand(M, parts, generator=g) + 0.5
            kw["rowsq"] = ((x_prev ** 2).sum(1, keepdim=True) * share / share.sum(1, keepdim=True)).cuda()
        if epi == STORE:
            kw["bias"] = (torch.randn(N, generator=g) * 0.1).cuda()
        else:
            kw.update(scale=(0.5 + torch.rand(N, generator=g)).cuda(), x=torch.randn(M, N, generator=g).cuda(),
                      next_w=(1.0 + 0.1 * torch.randn(N, generator=g)).cuda())
        _acts.clear()
        _acts[key] = (a, kw)
    return (_acts[key][0], _weights[(N, K)], _acts[key][1])


def call(ctx, a, w, epi, row_off, kw, lo=0, hi=None):
    """rt_debug_gemm_col on rows [lo, hi) of the operands, placed at row_off + lo; cut to what the launch writes (the rowsq row has
    tiles x 2 partials in every form: the layout is the callers')."""
    hi = a.shape[0] if hi is None else hi
    sl = lambda t: None if t is None else t[lo:hi].contiguous()
    res = run_col(ctx, a[lo:hi].contiguous(), w, epi, 0, row_off + lo, 1, sl(kw.get("rowsq")), 1e-6, kw.get("bias"), kw.get("scale"),
                  sl(kw.get("x")), kw.get("next_w"))
    N = w.shape[0]
    out = {}
    for k in KEYS:
        if res[k] is not None:
            out[k] = res[k][: (hi - lo) * ((N + 15) // 16) * 2] if k == "rowsq_out" else res[k]
    return out


def assert_same(got, ref, what):
    assert set(got) == set(ref) and got, what
    for k in got:
        assert not bool(torch.isnan(got[k].float()).any()), (what, k)
        assert torch.equal(got[k], ref[k]), (what, k)


@pytest.mark.parametrize("K", DEPTHS)
@pytest.mark.parametrize("M", ROWS)
def test_tile_blocked_launches_equal_the_half_tile_launch_bit_for_bit(ctx, M, K):
    """3702 against 3700 and 3701 against 3700 on out, next and rowsq_out, at row offsets 0 and 16."""
    for N in widths(ctx):
        for epi, parts in FORMS:
            a, w, kw = operands(M, K, N, epi, parts)
            for row_off in (0, 16):
                res = {}
                for value in (0, 1, 2):
                    switch(ctx, 3700 + value)
                    assert tile_rows(ctx, M, N, epi) == expected_block(M, value), (epi, N, M, value)
                    assert ctx.lib.rt_debug_col_row_blocks(n_cu(ctx), M, N, epi, 0) == 0       # (not a launch of the row-block rule)
                    res[value] = call(ctx, a, w, epi, row_off, kw)
                assert tile_rows(ctx, M, N, epi) in (16, 32)                   # (under 3702 every case of this test takes the form)
                assert_same(res[2], res[0], (epi, N, parts, row_off, "3702 against 3700"))
                assert_same(res[1], res[0], (epi, N, parts, row_off, "3701 against 3700"))
                assert float(res[2]["out"].abs().max()) > 1e-3                 # (the comparison is not one of zeros)
                if epi == RESID:
                    rq = res[2]["rowsq_out"].view(M, -1)
                    assert bool((rq > 0).all()), (N, row_off)                  # (every half-tile partial of every row was stored)


@pytest.mark.parametrize("K", DEPTHS)
@pytest.mark.parametrize("M", [32, 64, 24, 49])
def test_tile_blocked_launch_equals_one_launch_per_block(ctx, M, K):
    """A blocked 64-row launch == two 32-row launches at row_off and row_off + 32, a blocked 32-row launch == two 16-row launches
    (half-tile launches, as they exist without the switch); ragged last blocks (49 = 32 + 17, 24 = 16 + 8) as well."""
    blk = 32 if M > 32 else 16
    for N in widths(ctx):
        for epi, parts in FORMS:
            a, w, kw = operands(M, K, N, epi, parts)
            for row_off in (0, 16):
                switch(ctx, 3702)
                assert tile_rows(ctx, M, N, epi) == blk
                one = call(ctx, a, w, epi, row_off, kw)
                switch(ctx, 3700)
                assert tile_rows(ctx, blk, N, epi) == 0 and tile_rows(ctx, M - blk, N, epi) == 0
                lo, hi = call(ctx, a, w, epi, row_off, kw, 0, blk), call(ctx, a, w, epi, row_off, kw, blk, M)
                assert_same(one, {k: torch.cat([lo[k], hi[k]]) for k in lo}, (epi, N, parts, row_off, "one launch per block"))
    switch(ctx, 3702)


@pytest.mark.parametrize("K", DEPTHS)
@pytest.mark.parametrize("M", ROWS)
def test_small_integer_operands_are_exact(ctx, M, K):
    """|a|, |w| <= 4: every product and partial sum is an integer below 2^24, so the blocked STORE and RESID launches must equal
    the exact product whatever the summation order, and the rowsq row must sum to the row's sum of squares."""
    switch(ctx, 3702)
    a = ints((M, K), -4, 4, 3 + M)
    for N in widths(ctx):
        w = ints((N, K), -4, 4, 5 + N)
        ref = torch.from_numpy(a.float().numpy().astype(np.float64) @ w.float().numpy().astype(np.float64).T)
        assert float(ref.abs().max()) < 2 ** 24
        ref = ref.float().cuda()
        for epi in (STORE, RESID):
            assert tile_rows(ctx, M, N, epi) == expected_block(M, 2) != 0
            for row_off in (0, 16):
                if epi == STORE:
                    bias = ints((N,), -8, 8, 7).float().cuda()
                    got = call(ctx, a.cuda(), w.cuda(), STORE, row_off, dict(bias=bias))["out"]
                    assert torch.equal(got, ref + bias), (N, row_off)
                else:
                    x0 = ints((M, N), -16, 16, 9).float().cuda()
                    kw = dict(scale=torch.full((N,), 0.25, device="cuda"), x=x0, next_w=torch.full((N,), 2.0, device="cuda"))
                    r = call(ctx, a.cuda(), w.cuda(), RESID, row_off, kw)
                    want = x0 + 0.25 * ref
                    assert torch.equal(r["out"], want), (N, row_off)
                    assert torch.equal(r["next"].float(), (2.0 * want).to(torch.bfloat16).float())
                    n_part = (N + 15) // 16 * 2
                    # (the sums of squares pass 2^24: float32 rounding of each 8-column partial, as in tests/test_gemm_col_gpu.py)
                    rq, want_sq = r["rowsq_out"].view(M, n_part).double().sum(1), (want.double() ** 2).sum(1)
                    assert float(((rq - want_sq).abs() / want_sq.clamp(min=1)).max()) < 1e-5, (N, row_off)


def test_sixteen_and_sixty_five_rows_are_unchanged(ctx):
    """M = 16 has nothing to deal out and M = 65 belongs to the 128-row launch: the query says so, and the launches are what
    they were (equal under every value of the switch)."""
    for M in (16, 65):
        for N in widths(ctx):
            for epi, parts in FORMS:
                a, w, kw = operands(M, 224, N, epi, parts)
                res = {}
                for value in (0, 1, 2):
                    switch(ctx, 3700 + value)
                    assert tile_rows(ctx, M, N, epi) == 0, (M, epi, N, value)
                    res[value] = call(ctx, a, w, epi, 0, kw)
                assert_same(res[2], res[0], (M, epi, N))
                assert_same(res[1], res[0], (M, epi, N))


def test_generation_is_byte_identical_with_and_without_tile_blocks(ctx):
    """One short seeded, sampled generation on 20 rows of a two-layer model whose talker is 16 x (n_cu / 2) wide (its o and down
    launches take 16-row tile blocks) under 3700 and under 3702: the same codes and the same waveform, byte for byte.  Every
    accepted switch advances the plan's epoch, so the frames are captured anew: this is the replayed path."""
    from rho_tts_amd import config, weights
    from rho_tts_amd._native_model import NativeModel, RtSampling
    hidden = 16 * (n_cu(ctx) // 2)
    cfg = dataclasses.replace(config.small("small-wide"), talker=config.TransformerDims(hidden=hidden, layers=2, heads=hidden // 128, kv_heads=hidden // 256, head_dim=128, inter=256))
    B, frames = 20, 3
    switch(ctx, 3702)
    assert tile_rows(ctx, B, hidden, RESID) == 16
    nm = NativeModel(ctx, cfg, max_batch=B)
    try:
        nm.load_state({k: v.cuda() for k, v in weights.synthetic_state(cfg, 789).items()})
        g = torch.Generator().manual_seed(5)
        nm.set_voice("english", None, torch.randn(cfg.talker.hidden, generator=g) * 0.05,
                     [int(v) for v in torch.randint(0, cfg.text_vocab - 64, (5,), generator=g)],
                     torch.randint(0, cfg.codec.codebook_size, (9, cfg.n_groups), generator=g))
        texts = [[10 + i, 11 + 2 * i, 12 + 3 * i] for i in range(B)]
        sp = RtSampling(1, 0.9, 50, 1.0, 1.05)
        res = {}
        for value in (0, 2):
            switch(ctx, 3700 + value)
            codes = nm.generate(texts, [frames] * B, sp, seed=123)
            res[value] = (codes, nm.code2wav(codes))
        assert len(res[0][0]) == B and all(int(c.shape[0]) == frames for c in res[0][0])
        assert len({tuple(c.flatten().tolist()) for c in res[0][0]}) > 1               # (the items really differ: sampled, not degenerate)
        for a, b in zip(res[0][0], res[2][0]):
            assert torch.equal(a, b)
        for a, b in zip(res[0][1], res[2][1]):
            assert a.numel() > 0 and float(a.abs().max()) > 0 and torch.equal(a, b)
    finally:
        nm.close()
