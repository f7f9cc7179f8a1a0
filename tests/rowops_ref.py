"""Float64 references of the row kernels (rho_tts_amd/csrc/rowops.hip) and of the tiled GEMM's epilogue (gemm.hip
tile_epilogue_e), written from the definitions in the kernel comments, a mirror of the fragment-tiled layout (common.h tile_off),
and the comparison helpers of tests/test_rowops_gpu.py and tests/test_gemm_epilogue_gpu.py.

Everything here runs on the CPU; tests/test_rowops_ref_cpu.py checks the references against oracle/model.py and checks that every
comparison helper rejects a reference with one minimal defect.  Integer-valued operands make a float64 reference exact in float32
as well, so `ref.float()` is then the bit pattern a correct kernel must produce."""
import math

import numpy as np
import torch

F64 = torch.float64
ACT_NONE, ACT_SILU, ACT_GELU, ACT_SNAKE, ACT_CLAMP1, ACT_ELU = range(6)


# ------------------------------------------------------------------------------------------ number formats
def bf16(x):
    """float32 -> bfloat16, round to nearest even (what v_cvt_pk_bf16_f32 does)."""
    return x.to(torch.float32).to(torch.bfloat16)


def planes(x):
    """The hi / lo operand planes of a float32 tensor: hi = bf16(x), lo = bf16(x - hi)."""
    x = x.to(torch.float32)
    hi = bf16(x)
    return hi, bf16(x - hi.float())


def bits(t):
    """The tensor's bit patterns as integers (so -0.0 != +0.0 and a NaN equals itself)."""
    t = t.detach().cpu().contiguous()
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()]) if t.is_floating_point() else t


# ------------------------------------------------------------------------------------------ the tiled layout
def tile_off(m, k, K):
    """common.h tile_off: element (m, k) of a [rows][K] matrix in the fragment-tiled layout (16-row x 32-column tiles, K % 32 == 0)."""
    m, k = np.asarray(m, dtype=np.int64), np.asarray(k, dtype=np.int64)
    return ((((m >> 4) * (K >> 5) + (k >> 5)) * 64 + ((((k >> 3) & 3) << 4) | (m & 15))) << 3) + (k & 7)


def tile_rows(x, fill):
    """Row-major x [M][H] placed into a tiled buffer of 16 * ceil(M / 16) rows whose other elements hold `fill` (a tensor of
    that many elements, or a scalar)."""
    M, H = x.shape
    rows = (M + 15) // 16 * 16
    out = fill.clone().reshape(-1) if torch.is_tensor(fill) else torch.full((rows * H,), fill, dtype=x.dtype)
    assert out.numel() == rows * H
    off = tile_off(np.arange(M)[:, None], np.arange(H)[None, :], H)
    out[torch.from_numpy(off.reshape(-1))] = x.reshape(-1)
    return out


# ------------------------------------------------------------------------------------------ comparison helpers
def check_bits(got, ref, what=""):
    """Bit-for-bit equality."""
    g, r = bits(got), bits(ref)
    assert g.shape == r.shape and g.dtype == r.dtype, (what, g.shape, r.shape, g.dtype, r.dtype)
    bad = g != r
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {bad.numel()} elements differ, first at {tuple(bad.nonzero()[0].tolist())}"


def check_close(got, ref, tol, what=""):
    """|got - ref| <= tol element-wise (tol: a number or a tensor of ref's shape); returns the largest error."""
    g, r = got.detach().cpu().to(F64), ref.detach().cpu().to(F64)
    assert g.shape == r.shape, (what, g.shape, r.shape)
    assert bool(torch.isfinite(g).all()), f"{what}: non-finite output"
    err = (g - r).abs()
    t = tol.detach().cpu().to(F64) if torch.is_tensor(tol) else torch.full_like(err, float(tol))
    over = err > t
    assert not bool(over.any()), (f"{what}: {int(over.sum())} elements over tolerance, worst error {float(err.max()):.3e} "
                                  f"against {float(t[over].min()):.3e} at {tuple(over.nonzero()[0].tolist())}")
    return float(err.max()) if err.numel() else 0.0


def check_rel(got, ref, rtol, what="", floor=0.0):
    """|got - ref| <= rtol * max(floor, max|ref|)."""
    return check_close(got, ref, rtol * max(floor, float(ref.detach().abs().max())), what)


def check_untouched(buf, sentinel, written, what=""):
    """Every element of `buf` outside the boolean mask `written` still holds the bit pattern of `sentinel` (a scalar tensor of
    buf's dtype, or a tensor of buf's shape)."""
    b = bits(buf)
    s = bits(sentinel.to(buf.dtype) if torch.is_tensor(sentinel) else torch.tensor(sentinel, dtype=buf.dtype))
    s = s.expand_as(b) if s.dim() == 0 or s.shape != b.shape else s
    bad = (b != s) & ~written.cpu()
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} elements nobody owns were overwritten, first at {tuple(bad.nonzero()[0].tolist())}"


# ------------------------------------------------------------------------------------------ row kernels
def add_rmsnorm_ref(x, slabs=None, slab_bias=None, scale=None, w=None, eps=1e-6):
    """x += scale * (sum_s slab[s] + slab_bias); xn = w * x * rsqrt(mean(x^2) + eps).  Returns (x_new, xn or None, scale * sum)."""
    x = x.to(F64)
    add = torch.zeros_like(x)
    if slabs is not None and slabs.shape[0] > 0:
        add = slabs.to(F64).sum(0)
        if slab_bias is not None:
            add = add + slab_bias.to(F64)
        if scale is not None:
            add = add * scale.to(F64)
        x = x + add
    xn = None
    if w is not None:
        xn = w.to(F64) * (x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps))
    return x, xn, add


def rowsq_ref(x, drop_last=False):
    """Sum of squares of every row (drop_last: the defect of a reduction that misses the row's last element)."""
    x = x.to(F64)
    return (x[:, :-1] if drop_last else x).pow(2).sum(-1)


def norm_tiled_rows_ref(x, rowsq, w, eps):
    x = x.to(F64)
    return w.to(F64) * (x * torch.rsqrt(rowsq.to(F64).sum(-1, keepdim=True) / x.shape[-1] + eps))


def gather_rows_ref(table, idx, nonzero_negative=False):
    """table[idx], a row of zeros for a negative index (nonzero_negative: the defect of reading row 0 instead)."""
    out = table.to(F64)[idx.clamp(min=0).long()]
    return out if nonzero_negative else torch.where((idx >= 0)[:, None], out, torch.zeros_like(out))


def embed_ref(tables, idx, add_vec=None, f32_table=None, add_rows=None, add_row_idx=None):
    """Row r = add_vec + add_rows[add_row_idx[r]] + f32_table[idx[r][0]] + sum_j tables[j][idx[r][j]]; negative indices add nothing.
    Returns (x, sum of |terms|)."""
    M = idx.shape[0]
    H = (tables[0] if tables else f32_table).shape[-1]
    x, mag = torch.zeros(M, H, dtype=F64), torch.zeros(M, H, dtype=F64)

    def add(t):
        nonlocal x, mag
        x, mag = x + t, mag + t.abs()
    if add_vec is not None:
        add(add_vec.to(F64)[None, :].expand(M, H))
    if add_rows is not None:
        ar = add_row_idx if add_row_idx is not None else torch.arange(M)
        add(gather_rows_ref(add_rows, ar))
    if f32_table is not None:
        add(gather_rows_ref(f32_table, idx[:, 0]))
    for j, t in enumerate(tables):
        add(gather_rows_ref(t.float(), idx[:, j]))
    return x, mag


def silu(v):
    return v / (1.0 + torch.exp(-v))


def silu_mul_ref(slabs, I):
    s = slabs.to(F64).sum(0)
    return silu(s[:, :I]) * s[:, I:]


def activation(v, act, a=None, ib=None):
    if act == ACT_SILU:
        return silu(v)
    if act == ACT_GELU:
        return 0.5 * v * (1.0 + torch.erf(v / math.sqrt(2.0)))
    if act == ACT_SNAKE:
        return v + ib.to(F64) * torch.sin(v * a.to(F64)).pow(2)
    if act == ACT_CLAMP1:
        return v.clamp(-1.0, 1.0)
    if act == ACT_ELU:
        return torch.where(v > 0, v, torch.expm1(v))
    return v


def reduce_slabs_ref(slabs, bias=None, act=ACT_NONE):
    v = slabs.to(F64).sum(0)
    if bias is not None:
        v = v + bias.to(F64)
    return activation(v, act)


def qkv_post_ref(slabs, heads, kv_heads, d, qw, kw, eps, cos, sin, pos):
    """slabs [S][M][(heads + 2 kv) d] -> q [M][heads][d], k, v [M][kv][d]: RMSNorm over d (q, k), rotate-half RoPE at pos (q, k)."""
    s = slabs.to(F64).sum(0)
    M = s.shape[0]
    s = s.view(M, heads + 2 * kv_heads, d)
    q, k, v = s[:, :heads], s[:, heads:heads + kv_heads], s[:, heads + kv_heads:]

    def norm(t, w):
        return t if w is None else w.to(F64) * (t * torch.rsqrt(t.pow(2).mean(-1, keepdim=True) + eps))

    def rope(t):
        if cos is None:
            return t
        c, sn = cos.to(F64)[pos.long()][:, None, :], sin.to(F64)[pos.long()][:, None, :]
        h = d // 2
        a, b = t[..., :h], t[..., h:]
        return torch.cat([a * c - b * sn, b * c + a * sn], dim=-1)
    return rope(norm(q, qw)), rope(norm(k, kw)), v.clone()


def code_embed_mean_ref(table, codes):
    """table [Q][codebook][H], codes [rows][Q] clamped to the codebook -> the mean over q."""
    Q, cb, H = table.shape
    c = codes.clamp(0, cb - 1).long()
    return torch.stack([table.to(F64)[q][c[:, q]] for q in range(Q)], 0).sum(0) / Q


def dwconv_ln_ref(x, w, b, lw, lb, eps, leak=False):
    """x [B][T][C]: causal depthwise conv k = 7 (w [7][C]) within each item, LayerNorm over C.  leak: the defect of a conv whose
    first six rows of an item read the end of the item before."""
    B, T, C = x.shape
    xx = x.to(F64).reshape(1, B * T, C) if leak else x.to(F64)
    pad = torch.cat([torch.zeros(xx.shape[0], 6, C, dtype=F64), xx], 1)
    y = b.to(F64) + sum(w.to(F64)[k] * pad[:, k:k + xx.shape[1]] for k in range(7))
    y = y.reshape(B, T, C)
    mean = y.mean(-1, keepdim=True)
    var = (y - mean).pow(2).mean(-1, keepdim=True)
    return (y - mean) * torch.rsqrt(var + eps) * lw.to(F64) + lb.to(F64)


def final_conv_ref(x, w, bias):
    """x [B][T][C] (= hi + lo), w [7][C], bias [1] -> (clamp(y, -1, 1), y, |bias| + sum |terms|), each [B][T]."""
    B, T, C = x.shape
    pad = torch.cat([torch.zeros(B, 6, C, dtype=F64), x.to(F64)], 1)
    terms = [w.to(F64)[k] * pad[:, k:k + T] for k in range(7)]
    y = sum(t.sum(-1) for t in terms) + bias.to(F64)
    mag = sum(t.abs().sum(-1) for t in terms) + bias.to(F64).abs()
    return y.clamp(-1.0, 1.0), y, mag


# ------------------------------------------------------------------------------------------ GEMM epilogue
def conv_ref(x, w, taps, dilation):
    """Causal dilated conv as the implicit GEMM reads it: x [B][T][Cin], w [N][taps * Cin] (tap-major) -> [B][T][N]; output row t
    reads rows t - (taps - 1 - tap) * dilation, zero in front of the item."""
    B, T, Cin = x.shape
    x, w = x.to(F64), w.to(F64)
    p = (taps - 1) * dilation
    pad = torch.cat([torch.zeros(B, p, Cin, dtype=F64), x], 1)
    return sum(pad[:, k * dilation:k * dilation + T] @ w[:, k * Cin:(k + 1) * Cin].T for k in range(taps))


def epilogue_ref(acc, bias=None, act=ACT_NONE, snake_a=None, snake_ib=None, scale=None, residual=None, act2=None, snake2_a=None,
                 snake2_ib=None, shift_columns=False):
    """out = act(acc + bias) * scale + residual; out2 = act2(out).  shift_columns: the defect of per-column constants read one
    column to the right."""
    def col(v):
        return None if v is None else (torch.roll(v, -1) if shift_columns else v).to(F64)
    v = acc.to(F64)
    if bias is not None:
        v = v + col(bias)
    v = activation(v, act, col(snake_a), col(snake_ib))
    if scale is not None:
        v = v * col(scale)
    if residual is not None:
        v = v + residual.to(F64)
    out2 = None if act2 is None else activation(v, act2, col(snake2_a), col(snake2_ib))
    return v, out2


# ------------------------------------------------------------------------------------------ inputs shared by the CPU and the GPU tests
def _randn(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float32)


def dwconv_case(C, T, B=2):
    """Depthwise conv + LayerNorm input whose item 0 is loud, so a conv that read across the item boundary would show in the first
    six rows of item 1 (tests/test_rowops_ref_cpu.py asserts that it does, by more than the GPU test's tolerance)."""
    x = _randn(B, T, C, seed=29)
    x[0] = x[0] * 4 + 3
    return x, _randn(7, C, seed=30), _randn(C, seed=31), 1 + 0.1 * _randn(C, seed=32), _randn(C, seed=33)


def final_conv_int_case(C, T, B=2):
    """Integer-valued input of the last conv whose planes are both in use (x = 256 a + b needs more than bf16's 8 bits), integer
    weights and bias times ONE power of two chosen so that samples saturate at both ends and others land strictly inside: every
    product and partial sum is a multiple of that power of two below 2^24 of them - exact in float32 in any order."""
    g = torch.Generator().manual_seed(1000 + C)
    x = (256 * torch.randint(-2, 3, (B, T, C), generator=g) + torch.randint(-3, 4, (B, T, C), generator=g)).float()
    s = 2.0 ** -round(math.log2(math.sqrt(7 * C) * 400))
    w = torch.randint(-2, 3, (7, C), generator=g).float() * s
    return x, w, torch.tensor([3.0 * s])
