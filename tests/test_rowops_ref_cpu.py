"""CPU checks of tests/rowops_ref.py: the float64 references agree with oracle/model.py, the tile_off mirror is a bijection, and
every comparison helper of the GPU tests rejects a reference with ONE minimal defect - so a kernel with that defect could not pass
tests/test_rowops_gpu.py / tests/test_gemm_epilogue_gpu.py."""
import numpy as np
import pytest
import torch

from oracle import model as O
from tests import rowops_ref as R

F64 = torch.float64


def rnd(*shape, seed=0, dtype=F64):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=dtype)


def rejects(fn, *args, **kw):
    with pytest.raises(AssertionError):
        fn(*args, **kw)


# ------------------------------------------------------------------------------------------ against the oracle
def test_rmsnorm_reference_matches_oracle():
    x, w = rnd(3, 96, seed=1), rnd(96, seed=2)
    _, xn, _ = R.add_rmsnorm_ref(x, w=w, eps=1e-6)
    assert float((xn - O.rms_norm(x, w, 1e-6)).abs().max()) < 1e-13
    slabs, bias, scale = rnd(3, 3, 96, seed=3), rnd(96, seed=4), rnd(96, seed=5)
    x2, xn2, add = R.add_rmsnorm_ref(x, slabs, bias, scale, w, 1e-6)
    want = x + scale * (slabs.sum(0) + bias)
    assert float((x2 - want).abs().max()) < 1e-13 and float((add - (want - x)).abs().max()) < 1e-13
    assert float((xn2 - O.rms_norm(want, w, 1e-6)).abs().max()) < 1e-13
    assert float((R.norm_tiled_rows_ref(x, torch.stack([R.rowsq_ref(x), torch.zeros(3, dtype=F64)], 1), w, 1e-6) - O.rms_norm(x, w, 1e-6)).abs().max()) < 1e-13


def test_qkv_post_reference_matches_oracle_rms_norm_and_rope():
    heads, kv, d, M, max_pos = 4, 2, 32, 5, 16
    slabs = rnd(3, M, (heads + 2 * kv) * d, seed=6)
    qw, kw = rnd(d, seed=7), rnd(d, seed=8)
    ang = rnd(max_pos, d // 2, seed=9)
    cos, sin = torch.cos(ang), torch.sin(ang)
    pos = torch.tensor([0, 3, 15, 7, 7])
    q, k, v = R.qkv_post_ref(slabs, heads, kv, d, qw, kw, 1e-6, cos, sin, pos)
    s = slabs.sum(0).view(M, heads + 2 * kv, d)
    c, sn = cos[pos][:, None, :], sin[pos][:, None, :]
    assert float((q - O.apply_rope(O.rms_norm(s[:, :heads], qw, 1e-6), c, sn)).abs().max()) < 1e-13
    assert float((k - O.apply_rope(O.rms_norm(s[:, heads:heads + kv], kw, 1e-6), c, sn)).abs().max()) < 1e-13
    assert torch.equal(v, s[:, heads + kv:])
    q0, k0, _ = R.qkv_post_ref(slabs, heads, kv, d, None, None, 1e-6, None, None, pos)
    assert torch.equal(q0, s[:, :heads]) and torch.equal(k0, s[:, heads:heads + kv])


def test_conv_references_match_oracle_causal_conv1d():
    B, T, C = 2, 11, 8
    x = rnd(B, T, C, seed=10)
    # depthwise k = 7 (LayerNorm taken off by comparing before it: lw = 1, lb = 0 and an own LayerNorm of the oracle's conv)
    w, b, lw, lb = rnd(7, C, seed=11), rnd(C, seed=12), rnd(C, seed=13), rnd(C, seed=14)
    y = O.causal_conv1d(x.transpose(1, 2), w.T[:, None, :].contiguous(), b, groups=C).transpose(1, 2)
    want = torch.nn.functional.layer_norm(y, (C,), lw, lb, 1e-5)
    assert float((R.dwconv_ln_ref(x, w, b, lw, lb, 1e-5) - want).abs().max()) < 1e-12
    # dilated conv as the implicit GEMM reads it, and the last conv of the codec decoder
    for dil in (1, 3):
        wc = rnd(5, C, 7, seed=15)                                     # torch layout [N][Cin][k]
        wm = wc.permute(0, 2, 1).reshape(5, 7 * C)                      # tap-major rows
        ref = O.causal_conv1d(x.transpose(1, 2), wc, None, dilation=dil).transpose(1, 2)
        assert float((R.conv_ref(x, wm, 7, dil) - ref).abs().max()) < 1e-12
    wf, bf = rnd(7, C, seed=16), rnd(1, seed=17)
    yc, y, mag = R.final_conv_ref(x, wf, bf)
    ref = O.causal_conv1d(x.transpose(1, 2), wf.T[None].contiguous(), bf)[:, 0]
    assert float((y - ref).abs().max()) < 1e-12 and float((yc - ref.clamp(-1, 1)).abs().max()) < 1e-12 and bool((mag >= y.abs() - 1e-12).all())


def test_snake_reference_matches_oracle():
    x, alpha, beta = rnd(2, 6, 9, seed=18), rnd(6, seed=19), rnd(6, seed=20)
    a, ib = torch.exp(alpha), 1.0 / (torch.exp(beta) + 1e-9)
    got = R.activation(x.transpose(1, 2), R.ACT_SNAKE, a, ib).transpose(1, 2)
    assert float((got - O.snake_beta(x, alpha, beta)).abs().max()) < 1e-13
    out, out2 = R.epilogue_ref(x.transpose(1, 2), act=R.ACT_SNAKE, snake_a=a, snake_ib=ib, act2=R.ACT_ELU)
    assert torch.equal(out, got.transpose(1, 2)) and float((out2 - torch.nn.functional.elu(out)).abs().max()) < 1e-13


# ------------------------------------------------------------------------------------------ the tiled layout
@pytest.mark.parametrize("H", [32, 96, 2048])
@pytest.mark.parametrize("M", [1, 16, 33])
def test_tile_off_mirror_is_a_bijection(M, H):
    rows = (M + 15) // 16 * 16
    off = R.tile_off(np.arange(rows)[:, None], np.arange(H)[None, :], H).reshape(-1)
    assert off.min() == 0 and off.max() == rows * H - 1 and np.unique(off).size == rows * H
    # 8 consecutive columns stay consecutive (the 16-byte accesses of the kernels), and a 16-row tile is one contiguous block
    assert np.array_equal(R.tile_off(5, np.arange(8) + 40 % H, H) - R.tile_off(5, 40 % H, H), np.arange(8))
    assert np.array_equal(np.sort(off.reshape(rows, H)[:16].reshape(-1)), np.arange(16 * H))


def test_tile_rows_places_rows_and_keeps_the_fill():
    x = torch.arange(33 * 96, dtype=torch.float32).reshape(33, 96)
    t = R.tile_rows(x, -7.0)
    assert int((t == -7.0).sum()) == 15 * 96
    assert float(t[int(R.tile_off(32, 95, 96))]) == float(x[32, 95]) and float(t[int(R.tile_off(17, 8, 96))]) == float(x[17, 8])


# ------------------------------------------------------------------------------------------ sensitivity of the comparison helpers
def test_relative_check_rejects_a_sum_of_squares_without_the_row_s_last_element():
    x = rnd(3, 32, seed=21, dtype=torch.float32)
    x[:, -1] = x[:, -1].abs() + 0.05                      # (no accidental zero in the last column)
    ref = R.rowsq_ref(x)
    R.check_rel(ref.float(), ref, 1e-5)
    rejects(R.check_rel, R.rowsq_ref(x, drop_last=True).float(), ref, 1e-5)
    # ... and through the normalised output, at the GPU test's tolerance
    w = torch.ones(32)
    good = R.norm_tiled_rows_ref(x, ref[:, None], w, 1e-6)
    rejects(R.check_rel, R.norm_tiled_rows_ref(x, R.rowsq_ref(x, drop_last=True)[:, None], w, 1e-6), good, 1e-5)


def test_bit_check_rejects_two_rows_swapped_inside_a_tile():
    x = rnd(33, 96, seed=22, dtype=torch.float32)
    good = R.tile_rows(x, 0.0)
    R.check_bits(good.clone(), good)
    y = x.clone()
    y[[17, 18]] = x[[18, 17]]
    rejects(R.check_bits, R.tile_rows(y, 0.0), good)
    rejects(R.check_bits, R.tile_rows(R.bf16(y), 0.0), R.tile_rows(R.bf16(x), 0.0))


def test_checks_reject_per_column_constants_shifted_by_one_column():
    g = torch.Generator().manual_seed(23)
    acc = torch.randint(-20, 21, (5, 40), generator=g).to(F64)
    bias = torch.randint(-3, 4, (40,), generator=g).to(F64)
    bias[1] = bias[0] + 1                                 # (the shift is visible whatever the draw)
    scale = torch.tensor([1.0, 2.0, 0.5, 4.0]).repeat(10)
    good, _ = R.epilogue_ref(acc, bias=bias, scale=scale)
    for kw in ({"bias": bias}, {"scale": scale}):
        bad, _ = R.epilogue_ref(acc, **{"bias": bias, "scale": scale, **{k: torch.roll(v, -1) for k, v in kw.items()}})
        rejects(R.check_bits, bad.float(), good.float())
    # the arithmetic form: random constants, SnakeBeta on both outputs, at the GPU test's tolerance
    accr, a, ib = rnd(5, 40, seed=24) * 3, 0.5 + 1.5 * torch.rand(40, generator=g), 0.2 + 1.8 * torch.rand(40, generator=g)
    kw = dict(bias=rnd(40, seed=25), act=R.ACT_SNAKE, snake_a=a, snake_ib=ib, scale=0.5 + torch.rand(40, generator=g), act2=R.ACT_SNAKE,
              snake2_a=a.flip(0), snake2_ib=ib.flip(0))
    o1, o2 = R.epilogue_ref(accr, **kw)
    b1, b2 = R.epilogue_ref(accr, shift_columns=True, **kw)
    R.check_rel(o1.float(), o1, 2e-4, floor=1.0)
    rejects(R.check_rel, b1, o1, 2e-4, floor=1.0)
    rejects(R.check_rel, b2, o2, 2e-4, floor=1.0)


def test_plane_checks_reject_one_zeroed_lo_element():
    v = rnd(7, 40, seed=26, dtype=torch.float32) * 3
    hi, lo = R.planes(v)
    assert float((hi.float() + lo.float() - v).abs().max()) <= 2.0 ** -16 * float(v.abs().max())
    bad = lo.clone()
    i = int(lo.float().abs().argmax())
    bad.view(-1)[i] = 0
    rejects(R.check_bits, bad, lo)
    tol = 2.0 ** -16 * v.abs().to(F64) + 1e-5 * float(v.abs().max())
    R.check_close(hi.float() + lo.float(), v, tol)
    rejects(R.check_close, hi.float() + bad.float(), v, tol)


def test_sentinel_check_rejects_one_overwritten_padding_element():
    T, stride, B = 9, 14, 2
    sent = torch.tensor(-1234.5)
    buf = torch.full((B, stride), float(sent))
    written = torch.zeros(B, stride, dtype=torch.bool)
    written[:, :T] = True
    buf[:, :T] = rnd(B, T, seed=27, dtype=torch.float32)
    R.check_untouched(buf, sent, written)
    bad = buf.clone()
    bad[1, T] = 0.0                                        # the first padding element behind the row
    rejects(R.check_untouched, bad, sent, written)
    # a bf16 plane with a row stride of ldc = N + 8, and a pattern that differs from the sentinel in sign only
    pl = torch.full((5, 48), 3.0, dtype=torch.bfloat16)
    wr = torch.zeros(5, 48, dtype=torch.bool)
    wr[:, :40] = True
    pl[2, 47] = -3.0
    rejects(R.check_untouched, pl, torch.tensor(3.0, dtype=torch.bfloat16), wr)


def test_bit_check_rejects_a_negative_index_row_that_is_not_zero():
    table = rnd(6, 32, seed=28, dtype=torch.float32)
    idx = torch.tensor([2, -1, 5, 0])
    good = R.gather_rows_ref(table, idx)
    assert torch.equal(good[1], torch.zeros(32, dtype=F64)) and torch.equal(good[3], table[0].double())
    rejects(R.check_bits, R.gather_rows_ref(table, idx, nonzero_negative=True).float(), good.float())
    rejects(R.check_bits, R.rowsq_ref(R.gather_rows_ref(table, idx, nonzero_negative=True)).float(), R.rowsq_ref(good).float())
    # embed_ref: a negative index adds nothing
    x, mag = R.embed_ref([R.bf16(table), R.bf16(table)], torch.tensor([[1, -1], [-1, -1]]))
    assert torch.equal(x[0], R.bf16(table)[1].double()) and float(x[1].abs().max()) == 0.0 and torch.equal(mag[0], x[0].abs())


@pytest.mark.parametrize("C", [300, 1024])
@pytest.mark.parametrize("T", [1, 5, 8])
def test_relative_check_rejects_a_depthwise_conv_that_leaks_across_items(C, T):
    x, w, b, lw, lb = R.dwconv_case(C, T)
    good = R.dwconv_ln_ref(x, w, b, lw, lb, 1e-5)
    leak = R.dwconv_ln_ref(x, w, b, lw, lb, 1e-5, leak=True)
    assert torch.equal(leak[0], good[0])                   # item 0 has nothing in front of it
    n = min(T, 6)
    for t in range(n):                                     # each of the first six rows of item 1 sees item 0 in the defect
        rejects(R.check_close, leak[1, t], good[1, t], 1e-5 * float(good.abs().max()))
    rejects(R.check_rel, leak, good, 1e-5)
    if T > 6:
        assert float((leak[1, 6:] - good[1, 6:]).abs().max()) == 0.0


def test_final_conv_case_saturates_on_both_sides_and_stays_inside():
    for C in (16, 96, 112):
        x, w, bias = R.final_conv_int_case(C, 300)
        hi, lo = R.planes(x)
        assert torch.equal(hi.float() + lo.float(), x) and bool((lo.float() != 0).any())
        yc, y, _ = R.final_conv_ref(x, w, bias)
        assert bool((y > 1).any()) and bool((y < -1).any()) and bool(((y.abs() < 1) & (y != 0)).any())
        assert torch.equal(y.float().double(), y)          # the pre-clamp sums are exact in float32
