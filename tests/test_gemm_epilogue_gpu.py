"""The epilogue of the tiled GEMM and of k_conv_win (gemm.hip tile_epilogue_e) field by field, through rt_debug_gemm_epi, which
hands launch_gemm the whole GemmEpi: every activation, the per-column scale, the in-place residual, every output kind and the
second output, row strides above N, the XCD-aware tile order with its padded grid, and the fused conv pair.

Structure tests use integer-valued operands and snake_ib = 0 (the SnakeBeta term is then 0 * sin^2 = 0), so the float64 reference
of tests/rowops_ref.py is exact in float32 and every output is compared bit for bit - one wrong column tile, one plane at the
wrong 2-byte offset or one padding element written cannot hide.  Arithmetic tests use random operands against float64 at
2e-4 * max(1, max|ref|), the bar test_causal_dilated_conv_on_operand_planes sets for this kernel family."""
import pytest
import torch

from rho_tts_amd._native_model import RtDebugEpi
from tests import rowops_ref as R
from tests.rowops_ref import ACT_CLAMP1, ACT_ELU, ACT_GELU, ACT_NONE, ACT_SILU, ACT_SNAKE

pytestmark = pytest.mark.gpu

F64 = torch.float64
SENT = -77.0
PAD_ROWS = 3
DEFAULT_KNOBS = (601, 1001, 1801, 2101, 2601, 3001)
OUT_KINDS = {"out_f32": torch.float32, "out_bf16": torch.bfloat16, "out_hi": torch.bfloat16, "out_lo": torch.bfloat16,
             "out2_f32": torch.float32, "out2_bf16": torch.bfloat16, "out2_hi": torch.bfloat16, "out2_lo": torch.bfloat16}


@pytest.fixture(scope="module")
def ctx():
    from rho_tts_amd import _native
    c = _native.Context(0)
    yield c
    c.close()


def tune(ctx, *codes):
    for c in codes:
        assert ctx.lib.rt_debug_tune(c, 0) == 0, c


def gen(seed):
    return torch.Generator().manual_seed(seed)


def randn(*shape, seed):
    return torch.randn(*shape, generator=gen(seed), dtype=torch.float32)


def randint(lo, hi, *shape, seed):
    return torch.randint(lo, hi + 1, shape, generator=gen(seed)).float()


def uniform(lo, hi, *shape, seed):
    return lo + (hi - lo) * torch.rand(*shape, generator=gen(seed), dtype=torch.float32)


def a_operand(a, form):
    """The device form of a float32 activation: 0 bf16, 1 / 2 float32 (2: split on load), 3 the hi plane followed by the lo plane."""
    if form == 0:
        return R.bf16(a).cuda()
    if form == 3:
        hi, lo = R.planes(a)
        return torch.stack([hi, lo]).contiguous().cuda()
    return a.contiguous().cuda()


class Epi:
    """One epilogue: the per-column vectors, the residual ("alias": out_f32 itself, a tensor: a buffer of its own) and the outputs
    asked for, each [M + PAD_ROWS][ldc] and full of sentinels."""

    def __init__(self, M, N, outs, ldc=None, bias=None, scale=None, residual=None, act=ACT_NONE, snake=None, act2=ACT_SNAKE, snake2=None):
        self.M, self.N, self.ldc = M, N, ldc or N
        self.bias, self.scale, self.act, self.act2, self.snake, self.snake2 = bias, scale, act, act2, snake, snake2
        self.res = None if residual is None else (residual[0] if isinstance(residual, tuple) else residual)
        self.alias = isinstance(residual, tuple)
        self.bufs = {k: torch.full((M + PAD_ROWS, self.ldc), SENT, dtype=OUT_KINDS[k], device="cuda") for k in outs}
        self.keep = {}
        if self.res is not None:
            if self.alias:
                assert "out_f32" in self.bufs
                self.bufs["out_f32"][:M, :N] = self.res.cuda()
            else:
                r = torch.full((M + PAD_ROWS, self.ldc), SENT, dtype=torch.float32)
                r[:M, :N] = self.res
                self.keep["res"] = r.cuda()

    def struct(self):
        e = RtDebugEpi()
        d = lambda t: None if t is None else self.keep.setdefault(id(t), t.contiguous().cuda()).data_ptr()     # noqa: E731
        e.bias, e.scale = d(self.bias), d(self.scale)
        if self.res is not None:
            e.residual = self.bufs["out_f32"].data_ptr() if self.alias else self.keep["res"].data_ptr()
        for k, b in self.bufs.items():
            setattr(e, k, b.data_ptr())
        if self.snake is not None:
            e.snake_a, e.snake_ib = d(self.snake[0]), d(self.snake[1])
        if self.snake2 is not None:
            e.snake2_a, e.snake2_ib = d(self.snake2[0]), d(self.snake2[1])
        e.ldc, e.act, e.act2 = self.ldc, self.act, self.act2
        return e

    def ref(self, acc):
        has2 = any(k.startswith("out2") for k in self.bufs)
        return R.epilogue_ref(acc, self.bias, self.act, *(self.snake or (None, None)), self.scale, self.res, self.act2 if has2 else None,
                              *(self.snake2 or (None, None)))

    def got(self, k):
        return self.bufs[k].cpu()[:self.M, :self.N]

    def check_untouched(self, what):
        written = torch.zeros(self.M + PAD_ROWS, self.ldc, dtype=torch.bool)
        written[:self.M, :self.N] = True
        for k, b in self.bufs.items():
            R.check_untouched(b.cpu(), SENT, written, f"{what}: {k} padding columns and rows >= M")
        if "res" in self.keep:
            r = self.keep["res"].cpu()
            R.check_bits(r[:self.M, :self.N], self.res, f"{what}: the residual is read only")
            R.check_untouched(r, SENT, written, f"{what}: residual padding")

    def check_exact(self, acc, what):
        """Every output bit for bit against the (exact) reference, and the rounding identities between them."""
        out, out2 = self.ref(acc)
        for pre, ref in (("out", out), ("out2", out2)):
            if ref is None:
                continue
            f = ref.float()
            assert torch.equal(f.to(F64), ref), "the reference is not exact in float32"
            hi, lo = R.planes(f)
            for k, want in ((pre + "_f32", f), (pre + "_bf16", R.bf16(f)), (pre + "_hi", hi), (pre + "_lo", lo)):
                if k in self.bufs:
                    R.check_bits(self.got(k), want, f"{what}: {k}")
        self.check_untouched(what)

    def check_close(self, acc, what, rtol=2e-4):
        """out_f32 / out2_f32 against float64; the 2-byte outputs are roundings of the kernel's own float32 values bit for bit."""
        out, out2 = self.ref(acc)
        errs = {}
        for pre, ref in (("out", out), ("out2", out2)):
            if ref is None or pre + "_f32" not in self.bufs:
                continue
            f = self.got(pre + "_f32")
            errs[pre] = R.check_rel(f, ref, rtol, f"{what}: {pre}_f32", floor=1.0) / max(1.0, float(ref.abs().max()))
            hi, lo = R.planes(f)
            for k, want in ((pre + "_bf16", R.bf16(f)), (pre + "_hi", hi), (pre + "_lo", lo)):
                if k in self.bufs:
                    R.check_bits(self.got(k), want, f"{what}: {k} = rounding of {pre}_f32")
        self.check_untouched(what)
        return errs


def gemm_epi(ctx, a_dev, form, M, cin, w, e, taps=1, dil=1, rows=0, w2=None, e2=None, pair_mode=0):
    wd = R.bf16(w).cuda()
    w2d = None if w2 is None else R.bf16(w2).cuda()
    es, es2 = e.struct(), (None if e2 is None else e2.struct())
    torch.cuda.synchronize()
    return ctx.lib.rt_debug_gemm_epi(ctx.handle, a_dev.data_ptr(), form, M, cin, taps, dil, -(taps - 1) * dil, rows, rows, wd.data_ptr(), w.shape[0], es,
                                     None if w2d is None else w2d.data_ptr(), es2, pair_mode)


def int_operands(M, N, K, seed, nonneg=False, big=False):
    """Integer A and W in [-2, 2] ([0, 2] where the activation must see non-negative values); big: A = 256 a + b, which needs both
    operand planes of the split-precision forms (|acc| stays below 2^24)."""
    lo = 0 if nonneg else -2
    a = randint(lo, 2, M, K, seed=seed)
    if big:
        a = 256 * a + randint(lo, 2, M, K, seed=seed + 1)
    return a, randint(lo, 2, N, K, seed=seed + 2)


# ================================================================================================ 1. structure, bit-exact
def structure_cases(M, N, seed):
    """(name, non-negative operands, Epi kwargs): the output combinations of code2wav.hip, voice.hip, stt.hip and model_stack.hip,
    and all outputs at once."""
    bias, biasp = randint(-5, 5, N, seed=seed), randint(0, 5, N, seed=seed)
    scale = 2.0 ** randint(-2, 2, N, seed=seed + 1)
    res, resp = randint(-300, 300, M, N, seed=seed + 2), randint(0, 300, M, N, seed=seed + 2)
    sn = (uniform(0.5, 2, N, seed=seed + 3), torch.zeros(N))
    sn2 = (uniform(0.5, 2, N, seed=seed + 4), torch.zeros(N))
    p2 = ("out2_hi", "out2_lo")
    return [
        ("f32", False, dict(outs=("out_f32",), bias=bias)),
        ("no bias", False, dict(outs=("out_f32",))),
        ("bf16", False, dict(outs=("out_bf16",), bias=bias)),
        ("clamp", False, dict(outs=("out_f32",), bias=bias, act=ACT_CLAMP1)),
        ("layer scale + in-place residual", False, dict(outs=("out_f32",), bias=bias, scale=scale, residual=(res,))),
        ("residual from another buffer", False, dict(outs=("out_f32",), bias=bias, residual=res)),
        ("snake planes", False, dict(outs=("out_hi", "out_lo"), bias=bias, act=ACT_SNAKE, snake=sn)),
        ("elu planes", True, dict(outs=("out_hi", "out_lo"), bias=biasp, act=ACT_ELU)),
        ("snake2 planes only", False, dict(outs=p2, bias=bias, snake2=sn2)),
        ("f32 + snake2 planes", False, dict(outs=("out_f32",) + p2, bias=bias, snake2=sn2)),
        ("in-place residual + snake2 planes", False, dict(outs=("out_f32",) + p2, bias=bias, residual=(res,), snake2=sn2)),
        ("lean: residual, snake2 planes only", False, dict(outs=p2, bias=bias, residual=res, snake2=sn2)),
        ("in-place residual + elu2 planes", True, dict(outs=("out_f32",) + p2, bias=biasp, residual=(resp,), act2=ACT_ELU)),
        ("f32 + elu2 planes", True, dict(outs=("out_f32",) + p2, bias=biasp, act2=ACT_ELU)),
        ("everything", False, dict(outs=tuple(OUT_KINDS), bias=bias, scale=scale, residual=res, act=ACT_SNAKE, snake=sn, snake2=sn2)),
        ("everything, elu2", True, dict(outs=tuple(OUT_KINDS), bias=biasp, scale=scale, residual=resp, act=ACT_ELU, act2=ACT_ELU)),
    ]


@pytest.mark.parametrize("form", [0, 1, 2, 3])
@pytest.mark.parametrize("tile96", [600, 601])
@pytest.mark.parametrize("M,N,K", [(5, 40, 16), (130, 96, 64), (257, 288, 64), (300, 200, 96)])
def test_epilogue_structure_is_bit_exact(ctx, M, N, K, tile96, form):
    """Row and column tails of the 128 x 128 and the 128 x 96 tile, every A-operand form, ldc = N and N + 8.  The split-precision
    forms (2, 3) run three of the cases once more with A = 256 a + b, so that the low operand plane carries part of the value."""
    try:
        tune(ctx, tile96)
        for big in ((False, True) if form >= 2 else (False,)):
            ops = {nn: int_operands(M, N, K, seed=10 + nn, nonneg=bool(nn), big=big) for nn in (0, 1)}
            for ldc in (N, N + 8):
                for name, nonneg, kw in structure_cases(M, N, seed=20):
                    if big and name not in ("f32", "snake planes", "everything, elu2"):
                        continue
                    a, w = ops[int(nonneg)]
                    acc = a.to(F64) @ w.to(F64).T
                    e = Epi(M, N, ldc=ldc, **kw)
                    rc = gemm_epi(ctx, a_operand(a, form), form, M, K, w, e)
                    ctx.check(rc, "rt_debug_gemm_epi")
                    e.check_exact(acc, f"{name} ldc={ldc} big={big}")
    finally:
        tune(ctx, *DEFAULT_KNOBS)


def test_epilogue_refusals(ctx):
    a, w = int_operands(5, 40, 16, seed=1)
    ad = a_operand(a, 0)
    sn = (torch.ones(40), torch.zeros(40))
    for name, kw in (("hi without lo", dict(outs=("out_hi",))), ("out2_hi without out2_lo", dict(outs=("out2_hi",), snake2=sn)),
                     ("snake2 planes without constants", dict(outs=("out2_hi", "out2_lo"))), ("snake without constants", dict(outs=("out_f32",), act=ACT_SNAKE)),
                     ("ldc < N", dict(outs=("out_f32",), ldc=32)), ("unknown activation", dict(outs=("out_f32",), act=9))):
        e = Epi(5, 40, **kw)
        rc = gemm_epi(ctx, ad, 0, 5, 16, w, e)
        assert rc != 0, name
        for k, b in e.bufs.items():
            R.check_bits(b.cpu(), torch.full_like(b, SENT).cpu(), name)


# ================================================================================================ 2. arithmetic
MEASURED = {}


@pytest.mark.parametrize("M,N,K", [(130, 96, 64), (300, 200, 96)])
def test_epilogue_arithmetic(ctx, M, N, K, capsys):
    """Every act and every act2 on random operands (split-precision A, distinct random per-column bias / scale / snake constants in
    [0.5, 2] and [0.2, 2], pre-activations scaled to |v| <= 8) against float64 at 2e-4 * max(1, max|ref|).  The measured maxima,
    as a fraction of max(1, max|ref|), are printed."""
    a, w = randn(M, K, seed=1), R.bf16(randn(N, K, seed=2)).float()
    bias, scale = randn(N, seed=3), uniform(0.5, 2, N, seed=4)
    sn, sn2 = (uniform(0.5, 2, N, seed=5), uniform(0.2, 2, N, seed=6)), (uniform(0.5, 2, N, seed=7), uniform(0.2, 2, N, seed=8))
    res = randn(M, N, seed=9)
    a = a * (7.9 - float(bias.abs().max())) / float((a.to(F64) @ w.to(F64).T).abs().max())
    acc = a.to(F64) @ w.to(F64).T
    assert float((acc + bias.to(F64)).abs().max()) <= 8.0
    ad = a_operand(a, 2)
    for act in (ACT_NONE, ACT_SILU, ACT_GELU, ACT_SNAKE, ACT_CLAMP1, ACT_ELU):
        e = Epi(M, N, outs=("out_f32", "out_bf16", "out_hi", "out_lo"), ldc=N + 8, bias=bias, scale=scale, residual=(res,), act=act,
                snake=sn if act == ACT_SNAKE else None)
        ctx.check(gemm_epi(ctx, ad, 2, M, K, w, e), "rt_debug_gemm_epi")
        MEASURED[("act", act, M)] = e.check_close(acc, f"act {act}")["out"]
    for act2 in (ACT_SNAKE, ACT_ELU):
        e = Epi(M, N, outs=tuple(OUT_KINDS), ldc=N + 8, bias=bias, act2=act2, snake2=sn2 if act2 == ACT_SNAKE else None)
        ctx.check(gemm_epi(ctx, ad, 2, M, K, w, e), "rt_debug_gemm_epi")
        MEASURED[("act2", act2, M)] = e.check_close(acc, f"act2 {act2}")["out2"]
    with capsys.disabled():
        print("\nepilogue max error / max(1, max|ref|) at M=%d: " % M + ", ".join(f"{k[0]} {k[1]}: {v:.2e}" for k, v in MEASURED.items() if k[2] == M))


# ================================================================================================ 3. XCD tile order, grid padding
@pytest.mark.parametrize("N", [160, 192])
def test_xcd_tile_order_and_padded_grid(ctx, N):
    """M = 8200: 65 row tiles, so the XCD-aware order switches on and the launch pads the grid to 72 row tiles whose workgroups must
    do nothing.  Knob 1001 against 1000: bit-identical, equal to the reference, rows >= M untouched."""
    M, K = 8200, 64
    a, w = int_operands(M, N, K, seed=30)
    acc = a.to(F64) @ w.to(F64).T
    ad = a_operand(a, 0)
    kw = dict(outs=("out_f32", "out2_hi", "out2_lo"), bias=randint(-5, 5, N, seed=31), residual=(randint(-300, 300, M, N, seed=32),),
              snake2=(uniform(0.5, 2, N, seed=33), torch.zeros(N)))
    got = {}
    try:
        for code in (1001, 1000):
            tune(ctx, code)
            e = Epi(M, N, ldc=N + 8, **kw)
            ctx.check(gemm_epi(ctx, ad, 0, M, K, w, e), "rt_debug_gemm_epi")
            e.check_exact(acc, f"knob {code}")
            got[code] = {k: b.cpu() for k, b in e.bufs.items()}
    finally:
        tune(ctx, *DEFAULT_KNOBS)
    for k in got[1001]:
        R.check_bits(got[1001][k], got[1000][k], k)


def conv_int_case(B, T, cin, N, taps, seed, big=True):
    x = randint(-2, 2, B, T, cin, seed=seed)
    if big:
        x = 256 * x + randint(-2, 2, B, T, cin, seed=seed + 1)      # both planes in use
    return x, randint(-2, 2, N, taps * cin, seed=seed + 2)


def test_xcd_tile_order_through_the_window_conv(ctx):
    """The same through k_conv_win: operand planes, B = 2 x T = 4100 rows, 96 -> 192 channels, k = 7, dilation 3."""
    B, T, cin, N, taps, dil = 2, 4100, 96, 192, 7, 3
    x, w = conv_int_case(B, T, cin, N, taps, seed=40)
    acc = R.conv_ref(x, w, taps, dil).reshape(B * T, N)
    assert float(acc.abs().max()) < 2 ** 24
    xd = a_operand(x.reshape(B * T, cin), 3)
    kw = dict(outs=("out_f32", "out_hi", "out_lo"), bias=randint(-5, 5, N, seed=41), act=ACT_SNAKE, snake=(uniform(0.5, 2, N, seed=42), torch.zeros(N)))
    got = {}
    try:
        for code in (1001, 1000):
            tune(ctx, code)
            e = Epi(B * T, N, ldc=N + 8, **kw)
            ctx.check(gemm_epi(ctx, xd, 3, B * T, cin, w, e, taps=taps, dil=dil, rows=T), "rt_debug_gemm_epi")
            e.check_exact(acc, f"conv knob {code}")
            got[code] = {k: b.cpu() for k, b in e.bufs.items()}
    finally:
        tune(ctx, *DEFAULT_KNOBS)
    for k in got[1001]:
        R.check_bits(got[1001][k], got[1000][k], k)


# ================================================================================================ 4. fused conv pair
def pair_epis(M, C, form, lean, seed):
    """(first epilogue kwargs, second epilogue kwargs) of a residual unit: conv k = 7 + SnakeBeta, then 1x1 conv + residual +
    SnakeBeta planes; `lean`: no out_f32 (the residual is then read from a buffer of its own)."""
    if form == "int":
        b1, b2, res = randint(-5, 5, C, seed=seed), randint(-5, 5, C, seed=seed + 1), randint(-300, 300, M, C, seed=seed + 2)
        sn, sn2 = (uniform(0.5, 2, C, seed=seed + 3), torch.zeros(C)), (uniform(0.5, 2, C, seed=seed + 4), torch.zeros(C))
    else:
        b1, b2, res = randn(C, seed=seed), randn(C, seed=seed + 1), randn(M, C, seed=seed + 2)
        sn, sn2 = (uniform(0.5, 2, C, seed=seed + 3), uniform(0.2, 2, C, seed=seed + 5)), (uniform(0.5, 2, C, seed=seed + 4), uniform(0.2, 2, C, seed=seed + 6))
    e1 = dict(bias=b1, act=ACT_SNAKE, snake=sn)
    e2 = dict(outs=("out2_hi", "out2_lo") + (() if lean else ("out_f32",)), bias=b2, residual=res if lean else (res,), snake2=sn2)
    return e1, e2


def pair_ref(x, w1, w2, e1, taps, dil):
    B, T, C = x.shape
    mid = R.epilogue_ref(R.conv_ref(x, w1, taps, dil).reshape(B * T, -1), e1["bias"], ACT_SNAKE, *e1["snake"])[0]
    return mid, mid @ w2.to(F64).T


@pytest.mark.parametrize("lean", [False, True])
@pytest.mark.parametrize("T", [77, 129])
@pytest.mark.parametrize("dil", [1, 9])
@pytest.mark.parametrize("C", [96, 192])
def test_fused_conv_pair_structure(ctx, C, dil, T, lean):
    """Integers and snake_ib = 0: the intermediate is an integer below 2^16, so its hi + lo planes are exact and the whole unit is
    bit-exact against the reference and against the two-launch route through the planes; with knobs 2100 / 3000 conv_pair_fusable
    declines.  Also on the tall tile (1802) and the generic tap loop (2600) where launch_gemm admits them (192 channels fuse on the
    tap-unrolled kernel only: refused with 2600)."""
    B, taps = 3, 7
    M = B * T
    x, w1 = conv_int_case(B, T, C, C, taps, seed=50, big=False)
    w2 = randint(-2, 2, C, C, seed=53)
    e1kw, e2kw = pair_epis(M, C, "int", lean, seed=60)
    mid, acc2 = pair_ref(x, w1, w2, e1kw, taps, dil)
    assert float(mid.abs().max()) < 2 ** 16 and float(acc2.abs().max()) < 2 ** 23
    xd = a_operand(x.reshape(M, C), 3)
    try:
        fused = {}
        for knobs in ((), (1802,), (2600,), (1802, 2600)):
            tune(ctx, *DEFAULT_KNOBS)
            tune(ctx, *knobs)
            e1, e2 = Epi(M, C, outs=(), **e1kw), Epi(M, C, ldc=C + 8, **e2kw)
            rc = gemm_epi(ctx, xd, 3, M, C, w1, e1, taps=taps, dil=dil, rows=T, w2=w2, e2=e2, pair_mode=1)
            if C == 192 and 2600 in knobs:
                assert rc != 0, "192 channels on the generic tap loop"
                e1, e2 = Epi(M, C, outs=(), **e1kw), Epi(M, C, ldc=C + 8, **e2kw)
                assert gemm_epi(ctx, xd, 3, M, C, w1, e1, taps=taps, dil=dil, rows=T, w2=w2, e2=e2, pair_mode=2) != 0, "launch_gemm's own refusal"
                e2.check_untouched("refused pair")
                continue
            ctx.check(rc, "rt_debug_gemm_epi (fused pair)")
            e2.check_exact(acc2, f"fused C={C} dil={dil} T={T} knobs={knobs}")
            fused[knobs] = {k: b.cpu() for k, b in e2.bufs.items()}
        # the two-launch route: the fused form switched off is declined, then conv -> planes -> 1x1 conv
        tune(ctx, *DEFAULT_KNOBS)
        tune(ctx, 2100 if C == 96 else 3000)
        e1, e2 = Epi(M, C, outs=(), **e1kw), Epi(M, C, ldc=C + 8, **e2kw)
        assert gemm_epi(ctx, xd, 3, M, C, w1, e1, taps=taps, dil=dil, rows=T, w2=w2, e2=e2, pair_mode=1) != 0, "conv_pair_fusable with the pair switched off"
        e2.check_untouched("declined pair")
        mid_planes = torch.full((2, M, C), SENT, dtype=torch.bfloat16, device="cuda")
        e1 = Epi(M, C, outs=(), **e1kw)
        e1.bufs = {"out_hi": mid_planes[0], "out_lo": mid_planes[1]}
        ctx.check(gemm_epi(ctx, xd, 3, M, C, w1, e1, taps=taps, dil=dil, rows=T), "rt_debug_gemm_epi (conv)")
        hi, lo = R.planes(mid.float())
        R.check_bits(mid_planes[0].cpu(), hi, "intermediate hi plane")
        R.check_bits(mid_planes[1].cpu(), lo, "intermediate lo plane")
        e2 = Epi(M, C, ldc=C + 8, **e2kw)
        ctx.check(gemm_epi(ctx, mid_planes, 3, M, C, w2, e2), "rt_debug_gemm_epi (1x1 conv)")
        e2.check_exact(acc2, "two launches")
        for knobs, bufs in fused.items():
            for k, b in bufs.items():
                R.check_bits(b, e2.bufs[k].cpu(), f"fused {knobs} against two launches: {k}")
    finally:
        tune(ctx, *DEFAULT_KNOBS)


@pytest.mark.parametrize("T", [77, 129])
@pytest.mark.parametrize("dil", [1, 9])
@pytest.mark.parametrize("C", [96, 192])
def test_fused_conv_pair_arithmetic(ctx, C, dil, T, capsys):
    """Random operands: float64 reference of conv -> SnakeBeta -> 1x1 conv + residual -> SnakeBeta at 2e-4 * max(1, max|ref|)."""
    B, taps = 3, 7
    M = B * T
    x = randn(B, T, C, seed=70)
    w1, w2 = R.bf16(randn(C, taps * C, seed=71) * 0.03).float(), R.bf16(randn(C, C, seed=72) * 0.05).float()
    e1kw, e2kw = pair_epis(M, C, "rand", False, seed=80)
    mid, acc2 = pair_ref(x, w1, w2, e1kw, taps, dil)
    xd = a_operand(x.reshape(M, C), 3)
    x_planes = (xd[0].float().cpu().to(F64) + xd[1].float().cpu().to(F64)).reshape(B, T, C)
    mid, acc2 = pair_ref(x_planes, w1, w2, e1kw, taps, dil)            # (the reference reads what the planes hold)
    e1, e2 = Epi(M, C, outs=(), **e1kw), Epi(M, C, outs=("out_f32", "out2_f32", "out2_hi", "out2_lo"), ldc=C + 8,
                                              **{k: v for k, v in e2kw.items() if k != "outs"})
    ctx.check(gemm_epi(ctx, xd, 3, M, C, w1, e1, taps=taps, dil=dil, rows=T, w2=w2, e2=e2, pair_mode=1), "rt_debug_gemm_epi (fused pair)")
    errs = e2.check_close(acc2, f"fused pair C={C} dil={dil} T={T}")
    with capsys.disabled():
        print(f"\nfused pair C={C} dil={dil} T={T}: max error / max(1, max|ref|) out {errs['out']:.2e}, out2 {errs['out2']:.2e}")


def test_conv_pairs_the_launcher_cannot_fuse_return_its_status(ctx):
    B, T, taps = 2, 40, 7
    for C, act, name in ((128, ACT_SNAKE, "128 channels"), (96, ACT_ELU, "act != SnakeBeta"), (96, ACT_NONE, "no activation")):
        M = B * T
        x, w1 = conv_int_case(B, T, C, C, taps, seed=90, big=False)
        w2 = randint(-2, 2, C, C, seed=93)
        e1kw, e2kw = pair_epis(M, C, "int", False, seed=94)
        e1kw = dict(e1kw, act=act, snake=e1kw["snake"] if act == ACT_SNAKE else None)
        xd = a_operand(x.reshape(M, C), 3)
        for mode in (1, 2):
            e1, e2 = Epi(M, C, outs=(), **e1kw), Epi(M, C, ldc=C + 8, **e2kw)
            rc = gemm_epi(ctx, xd, 3, M, C, w1, e1, taps=taps, dil=1, rows=T, w2=w2, e2=e2, pair_mode=mode)
            assert rc != 0, f"{name}, pair_mode {mode}"
            e2.check_untouched(name)
