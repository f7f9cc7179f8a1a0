"""Row blocks of the column-owner decode GEMM (gemm_col.hip k_gemm_col, RB; rt_debug_tune 3600 / 3601 / 3602) through rt_debug_gemm_col.

A launch whose workgroups fill at most half of the CUs deals its rows over gridDim.y: 33..64 rows as two 32-row blocks (3601),
17..32 rows as two 16-row blocks as well (3602).  A row keeps its 8-wave K split, its k order inside a wave and the ww = 0..7 order of
the combine, so every output must equal the unblocked launch (3600) BIT FOR BIT - every comparison here is torch.equal.

Rows: each block edge and the ragged ends of both block sizes (17, 24, 31, 32 | 33, 47, 48, 49, 63, 64); 16 and 65 rows take no blocks.
K = 32 is one k-tile for eight waves (the guarded NPRE = 0 form), K = 224 fewer k-tiles than waves, K = 1024 a run of 4 (one fitted
chunk), K = 3072 a run of 12 (two chunks of 6).  RESID at N = 96 / 1024, STORE at N = 48 / 1024 without a row scale and with one
whose rowsq rows have 64 / 128 partials (the 16-byte requests of the wide prologue), SILU at N = 192 (the model's gate/up has too many
workgroups to qualify; here for the form).  rt_debug_col_row_blocks - the launcher's rule as host arithmetic - says for every case
which form it really took, so that no comparison is one of a launch with itself.
"""
import numpy as np
import pytest
import torch

from tests.test_gemm_col_gpu import RESID, SILU, STORE, ints, run_col, used_split

pytestmark = pytest.mark.gpu

ROWS = [17, 24, 31, 32, 33, 47, 48, 49, 63, 64]
DEPTHS = [32, 224, 1024, 3072]
# (epi, N, partials per rowsq row; 0 = no RMSNorm row scale)
FORMS = [(RESID, 96, 0), (RESID, 1024, 0), (STORE, 48, 0), (STORE, 48, 64), (STORE, 1024, 0), (STORE, 1024, 128), (SILU, 192, 64)]
KEYS = ("out", "next", "rowsq_out", "act")


@pytest.fixture(scope="module")
def ctx():
    from rho_tts_amd import _native
    c = _native.Context(0)
    yield c
    switch(c, 3600 + default_switch())
    c.close()


def default_switch():
    """The shipped value of the switch, from the one table of them."""
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rho_tts_amd", "csrc", "knobs.h")).read()
    return int(re.search(r"X\(3600, g_col_row_blocks, (\d+),", src).group(1))


def switch(ctx, code):
    assert ctx.lib.rt_debug_tune(code, 0) == 0, code


_device = {}


def block_rows(ctx, M, N, epi):
    """Rows per block of such a launch under the current switch (0: one workgroup per column tile has all the rows)."""
    if "n_cu" not in _device:
        _device["n_cu"] = ctx.device_info()["n_cu"]
    return ctx.lib.rt_debug_col_row_blocks(_device["n_cu"], M, N, epi, 0)


def expected_block(M, value):
    return 32 if (value >= 1 and 33 <= M <= 64) else 16 if (value >= 2 and 17 <= M <= 32) else 0


_operands = {}


def operands(M, K, N, epi, parts):
    """Random bf16 operands as a decode step has them, made once per shape and shared by every launch that is compared."""
    key = (M, K, N, epi, parts)
    if key not in _operands:
        g = torch.Generator().manual_seed(1000 * epi + N + K + 7 * M + parts)
        x_prev = torch.randn(M, K, generator=g)
        a = ((1.0 + 0.1 * torch.randn(K, generator=g)) * x_prev).to(torch.bfloat16).cuda()
        w = (torch.randn(N, K, generator=g) * 0.05).to(torch.bfloat16).cuda()
        kw = {}
        if parts:           # partial sums of squares whose total is the row's: a row scale of the usual size
            share = torch.rand(M, parts, generator=g) + 0.5
            kw["rowsq"] = ((x_prev ** 2).sum(1, keepdim=True) * share / share.sum(1, keepdim=True)).cuda()
        if epi == STORE:
            kw["bias"] = (torch.randn(N, generator=g) * 0.1).cuda()
        elif epi == RESID:
            kw.update(scale=(0.5 + torch.rand(N, generator=g)).cuda(), x=torch.randn(M, N, generator=g).cuda(),
                      next_w=(1.0 + 0.1 * torch.randn(N, generator=g)).cuda())
        _operands.clear()   # (one shape at a time: the cache serves the launches of one comparison)
        _operands[key] = (a, w, kw)
    return _operands[key]


def call(ctx, a, w, epi, row_off, kw, lo=0, hi=None):
    """rt_debug_gemm_col on rows [lo, hi) of the operands, placed at row_off + lo; cut to what the launch writes."""
    hi = a.shape[0] if hi is None else hi
    sl = lambda t: None if t is None else t[lo:hi].contiguous()
    res = run_col(ctx, a[lo:hi].contiguous(), w, epi, 0, row_off + lo, 1, sl(kw.get("rowsq")), 1e-6, kw.get("bias"), kw.get("scale"),
                  sl(kw.get("x")), kw.get("next_w"))
    N = w.shape[0]
    out = {}
    for k in KEYS:
        if res[k] is not None:
            out[k] = res[k][: (hi - lo) * ((N + 15) // 16) * used_split(ctx, N, 0)] if k == "rowsq_out" else res[k]
    return out


def assert_same(got, ref, what):
    assert set(got) == set(ref) and got, what
    for k in got:
        assert not bool(torch.isnan(got[k].float()).any()), (what, k)
        assert torch.equal(got[k], ref[k]), (what, k)


@pytest.mark.parametrize("K", DEPTHS)
@pytest.mark.parametrize("M", ROWS)
def test_blocked_launches_equal_the_unblocked_launch_bit_for_bit(ctx, M, K):
    """3602 against 3600 and 3601 against 3600 on out, next, rowsq_out and act, at row offsets 0 and 16."""
    for epi, N, parts in FORMS:
        a, w, kw = operands(M, K, N, epi, parts)
        for row_off in (0, 16):
            res = {}
            for value in (0, 1, 2):
                switch(ctx, 3600 + value)
                assert block_rows(ctx, M, N, epi) == expected_block(M, value), (epi, N, M, value)
                res[value] = call(ctx, a, w, epi, row_off, kw)
            assert block_rows(ctx, M, N, epi) in (16, 32)                  # (under 3602 every case of this test is a blocked launch)
            assert_same(res[2], res[0], (epi, N, parts, row_off, "3602 against 3600"))
            assert_same(res[1], res[0], (epi, N, parts, row_off, "3601 against 3600"))
            main = res[2]["act" if epi == SILU else "out"].float()
            assert float(main.abs().max()) > 1e-3                          # (the comparison is not one of zeros)


@pytest.mark.parametrize("K", DEPTHS)
@pytest.mark.parametrize("M", [32, 64, 24, 49])
def test_blocked_launch_equals_one_launch_per_block(ctx, M, K):
    """A blocked 64-row launch == two 32-row launches at row_off and row_off + 32, a blocked 32-row launch == two 16-row
    launches (the launches that exist without the switch); ragged last blocks (49 = 32 + 17, 24 = 16 + 8) as well."""
    blk = 32 if M > 32 else 16
    for epi, N, parts in FORMS:
        a, w, kw = operands(M, K, N, epi, parts)
        for row_off in (0, 16):
            switch(ctx, 3602)
            assert block_rows(ctx, M, N, epi) == blk
            one = call(ctx, a, w, epi, row_off, kw)
            switch(ctx, 3600)
            assert block_rows(ctx, blk, N, epi) == 0 and block_rows(ctx, M - blk, N, epi) == 0
            lo, hi = call(ctx, a, w, epi, row_off, kw, 0, blk), call(ctx, a, w, epi, row_off, kw, blk, M)
            assert_same(one, {k: torch.cat([lo[k], hi[k]]) for k in lo}, (epi, N, parts, row_off, "one launch per block"))
    switch(ctx, 3602)


@pytest.mark.parametrize("K", DEPTHS)
@pytest.mark.parametrize("M", ROWS)
def test_small_integer_operands_are_exact(ctx, M, K):
    """|a|, |w| <= 4: every product and partial sum is an integer below 2^24, so the blocked STORE and RESID launches must equal
    the exact product whatever the summation order."""
    switch(ctx, 3602)
    a = ints((M, K), -4, 4, 3 + M)
    for epi, N in ((STORE, 48), (STORE, 1024), (RESID, 96), (RESID, 1024)):
        assert block_rows(ctx, M, N, epi) == expected_block(M, 2) != 0
        w = ints((N, K), -4, 4, 5 + N)
        ref = torch.from_numpy(a.float().numpy().astype(np.float64) @ w.float().numpy().astype(np.float64).T)
        assert float(ref.abs().max()) < 2 ** 24
        ref = ref.float().cuda()
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
                n_part = (N + 15) // 16 * used_split(ctx, N, 0)
                # (the sums of squares pass 2^24: float32 rounding of each 16-column partial, as in tests/test_gemm_col_gpu.py)
                rq, want_sq = r["rowsq_out"].view(M, n_part).double().sum(1), (want.double() ** 2).sum(1)
                assert float(((rq - want_sq).abs() / want_sq.clamp(min=1)).max()) < 1e-5, (N, row_off)


def test_sixteen_and_sixty_five_rows_take_no_blocks(ctx):
    """M = 16 has nothing to deal out and M = 65 belongs to the 128-row launch: the query says so, and the launches are what
    they were (equal under every value of the switch)."""
    for M in (16, 65):
        for epi, N, parts in FORMS:
            a, w, kw = operands(M, 224, N, epi, parts)
            res = {}
            for value in (0, 2):
                switch(ctx, 3600 + value)
                assert block_rows(ctx, M, N, epi) == 0, (M, epi, N, value)
                res[value] = call(ctx, a, w, epi, 0, kw)
            assert_same(res[2], res[0], (M, epi, N))


def test_generation_is_byte_identical_with_and_without_row_blocks(ctx):
    """One short seeded generation of the small preset on 20 rows - the predictor's first pass has 40 rows (32-row blocks), every
    other decode GEMM 20 (16-row blocks) - under 3600 and under 3602: the same codes and the same waveform, byte for byte.  Every
    accepted switch advances the plan's epoch, so the frames are captured anew: this is the replayed path."""
    from rho_tts_amd import config, weights
    from rho_tts_amd._native_model import NativeModel, RtSampling
    cfg = config.small()
    B, frames = 20, 4
    switch(ctx, 3602)
    H, I = cfg.predictor.hidden, cfg.predictor.inter
    assert block_rows(ctx, 2 * B, H, RESID) == 32 and block_rows(ctx, B, H, RESID) == 16
    assert block_rows(ctx, B, cfg.talker.hidden, RESID) == 16 and block_rows(ctx, B, 2 * I, SILU) == 16
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
            switch(ctx, 3600 + value)
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
