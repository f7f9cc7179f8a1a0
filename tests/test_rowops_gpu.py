"""The row kernels of rho_tts_amd/csrc/rowops.hip one by one, through the rt_debug_* hooks that call their production launchers,
against the float64 references of tests/rowops_ref.py: bit for bit wherever the arithmetic is exact (integer-valued operands,
copies, roundings of the kernel's own float32 output), at a tolerance derived from the reduction's length otherwise.  The shapes
are the smallest that reach each branch of each kernel ("Kernel-level tests").  tests/test_rowops_ref_cpu.py shows
that every comparison used here rejects a reference with one minimal defect."""
import ctypes as C
import itertools

import pytest
import torch

from tests import rowops_ref as R

pytestmark = pytest.mark.gpu

F64 = torch.float64
EPS = 1e-6
SENT = -77.0                         # exact in bf16 and float32; no kernel output below equals it
U24 = 2.0 ** -24


@pytest.fixture(scope="module")
def ctx():
    from rho_tts_amd import _native
    c = _native.Context(0)
    yield c
    c.close()


def P(t):
    return None if t is None else t.data_ptr()


def dev(t):
    return None if t is None else t.contiguous().cuda()


def sent(*shape, dtype=torch.float32):
    return torch.full(shape, SENT, dtype=dtype, device="cuda")


def gen(seed):
    return torch.Generator().manual_seed(seed)


def randn(*shape, seed):
    return torch.randn(*shape, generator=gen(seed), dtype=torch.float32)


def randint(lo, hi, *shape, seed):
    return torch.randint(lo, hi + 1, shape, generator=gen(seed)).float()


def uniform(lo, hi, *shape, seed):
    return lo + (hi - lo) * torch.rand(*shape, generator=gen(seed), dtype=torch.float32)


def i32(values):
    return torch.tensor(values, dtype=torch.int32).cuda()


def tables_arg(tabs, strides):
    n = len(tabs)
    return (C.c_void_p * max(n, 1))(*[t.data_ptr() for t in tabs]), (C.c_int64 * max(n, 1))(*strides)


def refused(ctx, rc, what):
    assert rc != 0, f"{what}: launched instead of being refused"
    assert ctx.lib.rt_last_error(ctx.handle), what


# ================================================================================================ 1. add + RMSNorm
def add_rmsnorm(ctx, x, slabs, bias, scale, w, want_bf, want_f32):
    M, H = x.shape
    xd, o32, obf = dev(x).clone(), sent(M, H), sent(M, H, dtype=torch.bfloat16)
    n_slabs = 0 if slabs is None else slabs.shape[0]
    keep = [dev(slabs), dev(bias), dev(scale), dev(w)]
    torch.cuda.synchronize()
    rc = ctx.lib.rt_debug_add_rmsnorm(ctx.handle, P(xd), M, H, P(keep[0]), n_slabs, P(keep[1]), P(keep[2]), P(keep[3]), EPS,
                                      P(obf) if want_bf else None, P(o32) if want_f32 else None)
    return rc, xd.cpu(), o32.cpu(), obf.cpu()


@pytest.mark.parametrize("n_slabs", [0, 1, 3])
@pytest.mark.parametrize("M", [1, 3])
@pytest.mark.parametrize("H", [4, 96, 1024, 1028, 2048, 8192])
def test_add_rmsnorm(ctx, H, M, n_slabs):
    """k_add_rmsnorm (H = 4, 96; 1028 = 257 vectors, one lane runs a second round; 8192 = the limit, eight full rounds) and
    k_add_rmsnorm_v<1|2> (H = 1024, 2048).  The specialised kernels are compared with float64 at the generic kernel's tolerance,
    not with the generic kernel's bits: the generic kernel cannot be given the same row (two half-width problems have another
    mean square).

    Integer form (integer x / slabs / bias, power-of-two scale): the updated x is bit-exact.  Random form: x is normal, the addends
    (slabs, bias, scale) are positive, so no partial slab sum exceeds the total: a cancelling sum would round at the scale of its
    largest partial sum, which the bound 4 * 2^-24 * (|x| + |scale * sum|) - one fused multiply-add on top of the slab adds - does
    not see.  Normalised output: 1e-5 * max|ref| (at most 32 serial
    adds per lane, a 6-step wave tree and a 4-term sum: ~50 * 2^-24 = 3e-6, plus the reciprocal square root)."""
    w = 1 + 0.1 * randn(H, seed=4)
    for form in ("int", "rand"):
        if form == "int":
            x = randint(-8, 8, M, H, seed=1)
            slabs = randint(-8, 8, n_slabs, M, H, seed=2) if n_slabs else None
            bias, scale = randint(-4, 4, H, seed=3), 2.0 ** randint(-2, 2, H, seed=5)
        else:
            x = randn(M, H, seed=6)
            slabs = uniform(0.25, 1.0, n_slabs, M, H, seed=7) if n_slabs else None
            bias, scale = uniform(0.25, 1.0, H, seed=8), uniform(0.5, 2.0, H, seed=9)
        for use_b, use_s in ([(False, False)] if not n_slabs else itertools.product((False, True), repeat=2)):
            b, s = (bias if use_b else None), (scale if use_s else None)
            what = f"{form} H={H} M={M} slabs={n_slabs} bias={use_b} scale={use_s}"
            x_ref, xn_ref, add = R.add_rmsnorm_ref(x, slabs, b, s, w, EPS)
            rc, x_got, o32, obf = add_rmsnorm(ctx, x, slabs, b, s, w, True, True)
            ctx.check(rc, "rt_debug_add_rmsnorm")
            if not n_slabs:
                R.check_bits(x_got, x, what + ": x without slabs is left alone")
            elif form == "int":
                R.check_bits(x_got, x_ref.float(), what + ": updated x")
            else:
                R.check_close(x_got, x_ref, 4 * U24 * (x.to(F64).abs() + add.abs()), what + ": updated x")
            R.check_rel(o32, xn_ref, 1e-5, what + ": normalised f32")
            R.check_bits(obf, R.bf16(o32), what + ": out_bf16 is the rounding of out_f32")
            # either output alone, and the update alone (w == NULL): the same bits, and nothing else written
            for want_bf, want_f32, ww in ((True, False, w), (False, True, w), (False, False, w), (True, True, None)):
                rc, x2, o32b, obfb = add_rmsnorm(ctx, x, slabs, b, s, ww, want_bf, want_f32)
                ctx.check(rc, "rt_debug_add_rmsnorm")
                tag = f"{what} bf16={want_bf} f32={want_f32} w={'set' if ww is not None else 'NULL'}"
                R.check_bits(x2, x_got, tag + ": x")
                R.check_bits(o32b, o32 if (want_f32 and ww is not None) else sent(M, H).cpu(), tag + ": out_f32")
                R.check_bits(obfb, obf if (want_bf and ww is not None) else sent(M, H, dtype=torch.bfloat16).cpu(), tag + ": out_bf16")


@pytest.mark.parametrize("H", [6, 8196])
def test_add_rmsnorm_refuses_unsupported_widths(ctx, H):
    x = randn(2, H, seed=1)
    rc, x_got, o32, obf = add_rmsnorm(ctx, x, randn(1, 2, H, seed=2), None, None, torch.ones(H), True, True)
    refused(ctx, rc, f"H={H}")
    R.check_bits(x_got, x)
    R.check_bits(o32, sent(2, H).cpu())


# ================================================================================================ 2. k_rowsq / k_norm_tiled_rows
def rowsq(ctx, x, rowsq_n, norm_w=None, want_x=True, want_a=True, src=None, dst=None, out_rows=None, table=None, idx=None, idx_stride=1,
          first=0, frame=None, frame_stride=0, raw=False):
    M, H = x.shape
    out_rows = out_rows or M
    pad = (out_rows + 15) // 16 * 16 if raw else out_rows
    rs, xo, ao = sent(out_rows, rowsq_n), sent(pad, H), sent(pad, H, dtype=torch.bfloat16)
    keep = [dev(x), dev(norm_w), None if src is None else i32(src), None if dst is None else i32(dst), dev(table),
            None if idx is None else i32(idx), None if frame is None else i32([frame])]
    torch.cuda.synchronize()
    rc = ctx.lib.rt_debug_rowsq(ctx.handle, P(keep[0]), M, H, P(rs), rowsq_n, P(xo) if want_x else None, P(ao) if want_a else None, P(keep[1]),
                                P(keep[2]), P(keep[3]), out_rows, P(keep[4]), P(keep[5]), idx_stride, first, P(keep[6]), frame_stride, int(raw))
    return rc, rs.cpu(), xo.cpu(), ao.cpu()


def check_rowsq_outputs(x_rows, norm_w, rs, xo, ao, what, exact_sum):
    """x_rows: the float32 rows the kernel was to read, in output order."""
    ref = R.rowsq_ref(x_rows)
    if exact_sum:
        R.check_bits(rs[:, 0], ref.float(), what + ": sum of squares")
    else:
        R.check_rel(rs[:, 0], ref, 1e-5, what + ": sum of squares")
    R.check_bits(rs[:, 1:], torch.zeros_like(rs[:, 1:]), what + ": the other partial slots are +0")
    R.check_bits(xo, x_rows, what + ": f32 copy")
    R.check_bits(ao, R.bf16(norm_w * x_rows), what + ": bf16(norm_w * x)")


@pytest.mark.parametrize("rowsq_n", [1, 5])
@pytest.mark.parametrize("M", [1, 17, 33])
@pytest.mark.parametrize("H", [32, 1056])
def test_rowsq(ctx, H, M, rowsq_n):
    """k_rowsq: rows across 16-row tiles, H = 1056 = 264 vectors (a second round for eight lanes).  Sum of squares: exact for
    integer rows (every partial sum is an integer below 2^24), 1e-5 * max otherwise (at most 2 x 4 serial adds per lane, the wave
    tree, four terms); copies and the rounded operand bit for bit."""
    norm_w = 1 + 0.1 * randn(H, seed=2)
    for form, x in (("int", randint(-6, 6, M, H, seed=1)), ("rand", randn(M, H, seed=3))):
        rc, rs, xo, ao = rowsq(ctx, x, rowsq_n, norm_w)
        ctx.check(rc, "rt_debug_rowsq")
        check_rowsq_outputs(x, norm_w, rs, xo, ao, f"{form} H={H} M={M}", form == "int")
    # the sums alone (no tiled output): nothing else is written
    rc, rs2, xo, ao = rowsq(ctx, x, rowsq_n, None, want_x=False, want_a=False)
    ctx.check(rc, "rt_debug_rowsq")
    R.check_bits(rs2, rs, "sums alone")


@pytest.mark.parametrize("H", [32, 1056])
def test_rowsq_row_maps(ctx, H):
    """src_rows / dst_rows: a permutation with a repeated source row; output rows nobody writes keep their bytes."""
    M, out_rows = 17, 20
    x, norm_w = randint(-6, 6, M, H, seed=4), 1 + 0.1 * randn(H, seed=5)
    src = [(5 * i + 3) % M for i in range(M)]
    src[7] = src[2]                                            # a source row read twice
    dst = [(7 * i + 1) % out_rows for i in range(M)]           # distinct (7 and 20 are coprime), three rows left out
    rc, rs, xo, ao = rowsq(ctx, x, 5, norm_w, src=src, dst=dst, out_rows=out_rows)
    ctx.check(rc, "rt_debug_rowsq")
    written = torch.zeros(out_rows, dtype=torch.bool)
    written[dst] = True
    check_rowsq_outputs(x[src], norm_w, rs[dst], xo[dst], ao[dst], f"row maps H={H}", True)
    for buf in (rs, xo, ao):
        R.check_untouched(buf, SENT, written[:, None].expand_as(buf), "rows outside dst_rows")


@pytest.mark.parametrize("first_of", ["0", "M/2", "M"])
@pytest.mark.parametrize("M,H", [(17, 32), (6, 1056)])
def test_rowsq_gather(ctx, M, H, first_of):
    """Rows from `first` on come from an f32 table: index array at frame 2 (frame stride 50), index stride 2, one negative index
    (a row of zeros with sum 0)."""
    first = {"0": 0, "M/2": M // 2, "M": M}[first_of]
    V, frame, fs, stride = 9, 2, 50, 2
    x, table, norm_w = randint(-6, 6, M, H, seed=6), randint(-6, 6, V, H, seed=7), 1 + 0.1 * randn(H, seed=8)
    n_g = M - first
    ids = [(3 * j + 1) % V for j in range(n_g)]
    if n_g > 1:
        ids[1] = -1
    idx = torch.full((3 * fs,), 0, dtype=torch.int32)
    idx[:fs] = V - 1                                           # frame 0 / 1 entries are valid rows, but the wrong ones
    idx[fs:2 * fs] = V - 2
    for j, v in enumerate(ids):
        idx[frame * fs + j * stride] = v
    rc, rs, xo, ao = rowsq(ctx, x, 5, norm_w, table=table, idx=idx.tolist(), idx_stride=stride, first=first, frame=frame, frame_stride=fs)
    ctx.check(rc, "rt_debug_rowsq")
    rows = torch.cat([x[:first], R.gather_rows_ref(table, torch.tensor(ids, dtype=torch.long)).float().reshape(n_g, H)])
    check_rowsq_outputs(rows, norm_w, rs, xo, ao, f"gather first={first}", True)
    if n_g > 1:
        R.check_bits(rs[first + 1], torch.zeros(5), "negative index: sum 0")
        R.check_bits(xo[first + 1], torch.zeros(H), "negative index: a row of +0")


def test_rowsq_refuses_a_gather_with_row_maps(ctx):
    x, table = randn(4, 32, seed=1), randn(4, 32, seed=2)
    for kw in ({"src": [0, 1, 2, 3]}, {"dst": [0, 1, 2, 3]}, {"first": 5}):
        rc, rs, xo, ao = rowsq(ctx, x, 1, torch.ones(32), table=table, idx=[0, 1, 2, 3], **kw)
        refused(ctx, rc, str(kw))
        R.check_bits(rs, sent(4, 1).cpu())


@pytest.mark.parametrize("rowsq_n", [1, 300])
@pytest.mark.parametrize("M,H", [(1, 32), (17, 1056), (33, 32)])
def test_norm_tiled_rows(ctx, M, H, rowsq_n):
    """k_norm_tiled_rows: 300 partial sums make 44 lanes add a second one; float64 at 1e-5 * max|ref|."""
    x, w = randn(M, H, seed=9), 1 + 0.1 * randn(H, seed=10)
    parts = uniform(0.0, 2.0 * H / rowsq_n, M, rowsq_n, seed=11)
    xd, pd, wd, out = dev(x), dev(parts), dev(w), sent(M, H)
    torch.cuda.synchronize()
    ctx.check(ctx.lib.rt_debug_norm_tiled_rows(ctx.handle, P(xd), P(pd), rowsq_n, P(wd), EPS, M, H, P(out)), "rt_debug_norm_tiled_rows")
    R.check_rel(out.cpu(), R.norm_tiled_rows_ref(x, parts, w, EPS), 1e-5, f"M={M} H={H} n={rowsq_n}")


# ================================================================================================ 3. k_embed_rowsq
class Embed:
    """One problem of k_embed_rowsq: n_src bf16 tables (row stride H + 8) or an f32 table, an index array of `frames` frames."""

    def __init__(self, M, H, n_src, form, seed, f32_table=False, add_vec=True, extra_stride=2, frames=3, V=7):
        self.M, self.H, self.n_src, self.V, self.frames = M, H, n_src, V, frames
        mk = (lambda *s, seed: randint(-2, 2, *s, seed=seed)) if form == "int" else (lambda *s, seed: randn(*s, seed=seed))
        self.stride_el = H + 8
        self.tabs = [R.bf16(mk(V, self.stride_el, seed=seed + 10 + j)) for j in range(n_src)]
        self.f32_table = mk(V, H, seed=seed + 40) if f32_table else None
        self.add_vec = mk(H, seed=seed + 41) if add_vec else None
        self.norm_w = 1 + 0.1 * randn(H, seed=seed + 42)
        self.idx_stride = max(n_src, 1) + extra_stride
        self.fs = M * self.idx_stride + 3
        idx = torch.randint(0, V, (frames, self.fs), generator=gen(seed + 43), dtype=torch.int32)
        neg = torch.rand(frames, self.fs, generator=gen(seed + 44)) < 0.3
        idx[neg] = -1
        if n_src > 1:
            idx[:, 0] = 1                                       # row 0 keeps its first source in every frame
            idx[:, 1] = -2                                      # ... and skips its second one
        self.idx = idx
        self.d = dict(tabs=[dev(t) for t in self.tabs], f32=dev(self.f32_table), add=dev(self.add_vec), w=dev(self.norm_w), idx=dev(idx))

    def ref(self, frame):
        rows = self.idx[frame, :self.M * self.idx_stride].reshape(self.M, self.idx_stride).long()
        return R.embed_ref([t[:, :self.H] for t in self.tabs], rows, self.add_vec, self.f32_table)

    def run(self, ctx, frame_dev=None, frame_inc=False, arrive=None, qkv_table=None, qkv_out=None, qkv_n=0, raw=False, rowsq_n=3, n_src=None):
        M, H = self.M, self.H
        pad = (M + 15) // 16 * 16 if raw else M
        rs, xo, ao = sent(M, rowsq_n), sent(pad, H), sent(pad, H, dtype=torch.bfloat16)
        n_src = self.n_src if n_src is None else n_src
        tp, sp = tables_arg(self.d["tabs"][:n_src] if n_src <= len(self.d["tabs"]) else self.d["tabs"] * n_src, [self.stride_el] * max(n_src, 1))
        torch.cuda.synchronize()
        rc = ctx.lib.rt_debug_embed_rowsq(ctx.handle, tp, sp, n_src, P(self.d["f32"]), P(self.d["idx"]), self.idx_stride, P(frame_dev), self.fs, M, H,
                                          P(self.d["add"]), P(rs), rowsq_n, P(xo), P(ao), P(self.d["w"]), P(frame_dev) if frame_inc else None,
                                          P(arrive), P(qkv_table), P(qkv_out), qkv_n, int(raw))
        return rc, rs.cpu(), xo.cpu(), ao.cpu()

    def check(self, frame, rs, xo, ao, form, what):
        x_ref, mag = self.ref(frame)
        if form == "int":
            R.check_bits(xo, x_ref.float(), what + ": x")
            R.check_bits(rs[:, 0], R.rowsq_ref(x_ref).float(), what + ": sum of squares")
        else:
            R.check_close(xo, x_ref, 16 * U24 * mag, what + ": x")
            R.check_rel(rs[:, 0], R.rowsq_ref(x_ref), 1e-5, what + ": sum of squares")
        R.check_bits(rs[:, 1:], torch.zeros_like(rs[:, 1:]), what + ": the other partial slots")
        R.check_bits(ao, R.bf16(self.norm_w * xo), what + ": bf16(norm_w * x) of the kernel's own x")


@pytest.mark.parametrize("add_vec", [True, False])
@pytest.mark.parametrize("n_src", [1, 3, 16])
@pytest.mark.parametrize("H", [32, 2080])
def test_embed_rowsq_bf16_sources(ctx, H, n_src, add_vec):
    """Sums of bf16 embedding rows in source order, some indices negative (the source is skipped), index stride n_src + 2, the index
    array at frame 2; H = 2080 makes eight lanes run the loop's second round.  Small integers: exact, so x, the rounded operand and
    rowsq[0] are bit-exact (|x| <= 34, 2080 squares stay below 2^24).  Random: float64 at 16 * 2^-24 * sum|terms| (at most 17 adds)."""
    for form in ("int", "rand"):
        p = Embed(5, H, n_src, form, seed=100, add_vec=add_vec)
        rc, rs, xo, ao = p.run(ctx, frame_dev=i32([2]))
        ctx.check(rc, "rt_debug_embed_rowsq")
        p.check(2, rs, xo, ao, form, f"{form} H={H} n_src={n_src} add_vec={add_vec}")
    rc, rs, xo, ao = p.run(ctx, frame_dev=None)                 # no frame pointer: frame 0
    ctx.check(rc, "rt_debug_embed_rowsq")
    p.check(0, rs, xo, ao, form, "no frame pointer")


@pytest.mark.parametrize("add_vec", [True, False])
@pytest.mark.parametrize("H", [32, 2080])
def test_embed_rowsq_f32_table(ctx, H, add_vec):
    """n_src = 0: one row of an f32 table per output row (a negative index adds nothing)."""
    for form in ("int", "rand"):
        p = Embed(5, H, 0, form, seed=200, f32_table=True, add_vec=add_vec)
        rc, rs, xo, ao = p.run(ctx, frame_dev=i32([1]))
        ctx.check(rc, "rt_debug_embed_rowsq")
        p.check(1, rs, xo, ao, form, f"f32 table {form} H={H} add_vec={add_vec}")


@pytest.mark.parametrize("qkv_n", [4, 128, 4100])
@pytest.mark.parametrize("f32_table", [False, True])
def test_embed_rowsq_qkv_table(ctx, qkv_n, f32_table):
    """The q/k/v row of the row's code: 4100 floats = 1025 vectors, one past the 4 x 256 a workgroup preloads (the copy tail); a
    negative code reads row 0; rows are bit-identical to table rows and the guard behind the last row keeps its bytes."""
    p = Embed(5, 32, 0 if f32_table else 1, "int", seed=300, f32_table=f32_table)
    p.idx[0, 0], p.idx[0, p.idx_stride] = 3, -1                 # row 0: code 3, row 1: a negative code
    p.d["idx"] = dev(p.idx)
    table = randn(p.V, qkv_n, seed=301)
    td, out = dev(table), sent(5 * qkv_n + 64)
    rc, rs, xo, ao = p.run(ctx, qkv_table=td, qkv_out=out, qkv_n=qkv_n)
    ctx.check(rc, "rt_debug_embed_rowsq")
    p.check(0, rs, xo, ao, "int", f"qkv_n={qkv_n}")
    codes = p.idx[0, :5 * p.idx_stride:p.idx_stride].long()
    assert int(codes[0]) == 3 and int(codes[1]) == -1
    got = out.cpu()
    R.check_bits(got[:5 * qkv_n].reshape(5, qkv_n), table[codes.clamp(min=0)], "q/k/v rows")
    R.check_bits(got[5 * qkv_n:], torch.full((64,), SENT), "guard behind the last q/k/v row")


@pytest.mark.parametrize("M", [1, 5])
def test_embed_rowsq_advances_the_frame_counter_once(ctx, M):
    """frame_inc: after a launch of M workgroups the counter is +1 exactly and `arrive` is back at 0; the launch read its indices
    at the old frame, the next one reads the new frame."""
    p = Embed(M, 32, 3, "int", seed=400)
    p.idx[:, 2] = torch.tensor([2, 3, 4], dtype=torch.int32)    # row 0's third source differs from frame to frame
    p.d["idx"] = dev(p.idx)
    frame, arrive = i32([0]), torch.zeros(1, dtype=torch.int32, device="cuda")
    for f in (0, 1):
        rc, rs, xo, ao = p.run(ctx, frame_dev=frame, frame_inc=True, arrive=arrive)
        ctx.check(rc, "rt_debug_embed_rowsq")
        assert int(frame.cpu()) == f + 1 and int(arrive.cpu()) == 0, (f, int(frame.cpu()), int(arrive.cpu()))
        p.check(f, rs, xo, ao, "int", f"M={M} launch {f}")
        assert not torch.equal(p.ref(f)[0], p.ref(f + 1)[0])   # (the frames differ, so a launch at the wrong frame would show)


def test_embed_rowsq_refusals(ctx):
    frame, arrive = i32([0]), torch.zeros(1, dtype=torch.int32, device="cuda")
    qt, qo = dev(randn(7, 8, seed=1)), sent(5 * 8)
    pf = Embed(5, 32, 0, "int", seed=500, f32_table=True)
    refused(ctx, pf.run(ctx, frame_dev=frame, frame_inc=True, arrive=arrive)[0], "frame_inc with the f32 table")
    p3 = Embed(5, 32, 3, "int", seed=501)
    refused(ctx, p3.run(ctx, frame_dev=frame, frame_inc=True, arrive=None)[0], "frame_inc without an arrival counter")
    refused(ctx, p3.run(ctx, qkv_table=qt, qkv_out=qo, qkv_n=8)[0], "q/k/v table with three sources")
    refused(ctx, p3.run(ctx, n_src=17)[0], "17 sources")
    p1 = Embed(5, 32, 1, "int", seed=502)
    refused(ctx, p1.run(ctx, qkv_table=qt, qkv_out=qo, qkv_n=6)[0], "q/k/v width 6")
    refused(ctx, p1.run(ctx, qkv_table=qt, qkv_out=None, qkv_n=8)[0], "q/k/v table without an output")
    refused(ctx, p1.run(ctx, frame_dev=frame, frame_inc=True, arrive=arrive, qkv_table=qt, qkv_out=qo, qkv_n=8)[0], "q/k/v table with frame_inc")
    assert int(frame.cpu()) == 0 and int(arrive.cpu()) == 0
    R.check_bits(qo.cpu(), torch.full((40,), SENT))


# ================================================================================================ 4. layout
def test_tiled_layout_of_rowsq_and_embed_rowsq(ctx):
    """M = 33, H = 96: the raw tiled buffers equal the tile_off mirror's placement of the row-major result, and the elements of
    rows 33 .. 47 of the last tile keep their bytes."""
    M, H = 33, 96
    x, norm_w = randn(M, H, seed=1), 1 + 0.1 * randn(H, seed=2)
    rc, rs, xo, ao = rowsq(ctx, x, 1, norm_w, raw=True)
    ctx.check(rc, "rt_debug_rowsq")
    R.check_bits(xo.reshape(-1), R.tile_rows(x, SENT), "k_rowsq: tiled f32")
    R.check_bits(ao.reshape(-1), R.tile_rows(R.bf16(norm_w * x), torch.full((48 * H,), SENT, dtype=torch.bfloat16)), "k_rowsq: tiled bf16")
    assert int((xo == SENT).sum()) == 15 * H and int((ao == SENT).sum()) == 15 * H
    p = Embed(M, H, 3, "int", seed=600)
    rc, rs, xo, ao = p.run(ctx, raw=True)
    ctx.check(rc, "rt_debug_embed_rowsq")
    x_ref = p.ref(0)[0].float()
    R.check_bits(xo.reshape(-1), R.tile_rows(x_ref, SENT), "k_embed_rowsq: tiled f32")
    R.check_bits(ao.reshape(-1), R.tile_rows(R.bf16(p.norm_w * x_ref), torch.full((48 * H,), SENT, dtype=torch.bfloat16)), "k_embed_rowsq: tiled bf16")
    # the hook's row-major path is the same launch seen through k_untile_rows
    rc, rs2, xo2, ao2 = p.run(ctx)
    ctx.check(rc, "rt_debug_embed_rowsq")
    R.check_bits(xo2, x_ref, "row-major path")


# ================================================================================================ 5. elementwise kernels
def sample_idx(n, seed):
    return torch.cat([torch.tensor([0, n - 1]), torch.randint(0, n, (1000,), generator=gen(seed))])


@pytest.mark.parametrize("M,I,n_slabs", [(3, 4, 1), (3, 4, 3), (3, 100, 1), (3, 100, 3), (64, 32772, 1)])
def test_silu_mul(ctx, M, I, n_slabs):
    """k_silu_mul; 64 x 32772 / 4 vectors are 64 more than 8192 workgroups x 64 lanes hold: the grid-stride branch.  float32 output
    against float64 at 1e-5 * max|ref| over the whole tensor (three adds, the fast exponential, a division, a product), the first,
    the last and 1000 random elements named on their own; the bf16 output is the rounding of the float32 one bit for bit."""
    slabs = randn(n_slabs, M, 2 * I, seed=1)
    sd, o32, obf = dev(slabs), sent(M, I), sent(M, I, dtype=torch.bfloat16)
    torch.cuda.synchronize()
    ctx.check(ctx.lib.rt_debug_silu_mul(ctx.handle, P(sd), n_slabs, M, I, None, P(o32)), "rt_debug_silu_mul")
    ctx.check(ctx.lib.rt_debug_silu_mul(ctx.handle, P(sd), n_slabs, M, I, P(obf), None), "rt_debug_silu_mul")
    ref = R.silu_mul_ref(slabs, I)
    tol = 1e-5 * float(ref.abs().max())
    pick = sample_idx(M * I, 2)
    R.check_close(o32.cpu().reshape(-1)[pick], ref.reshape(-1)[pick], tol, f"M={M} I={I}: first, last and random elements")
    R.check_close(o32.cpu(), ref, tol, f"M={M} I={I}: whole tensor")
    R.check_bits(obf.cpu(), R.bf16(o32.cpu()), "bf16 output = rounding of the f32 output")


def test_silu_mul_refuses_an_odd_width(ctx):
    sd, o32 = dev(randn(1, 2, 12, seed=1)), sent(2, 6)
    torch.cuda.synchronize()
    refused(ctx, ctx.lib.rt_debug_silu_mul(ctx.handle, P(sd), 1, 2, 6, None, P(o32)), "I=6")
    R.check_bits(o32.cpu(), sent(2, 6).cpu())


@pytest.mark.parametrize("M,N,n_slabs", [(3, 4, 1), (3, 4, 3), (3, 100, 1), (3, 100, 3), (700, 3001, 3)])
def test_reduce_slabs(ctx, M, N, n_slabs):
    """k_reduce_slabs; 700 x 3001 elements are 3548 more than 8192 workgroups x 256 lanes: the grid-stride branch.  act = none with
    integer slabs and bias: bit-exact, to both outputs at once and to each alone.  SiLU / GELU: float64 at 1e-5 * max|ref|."""
    slabs, bias = randint(-9, 9, n_slabs, M, N, seed=1), randint(-9, 9, N, seed=2)
    sd, bd = dev(slabs), dev(bias)
    ref = R.reduce_slabs_ref(slabs, bias).float()
    for want32, wantbf, b in ((True, True, bd), (True, False, bd), (False, True, bd), (True, False, None)):
        o32, obf = sent(M, N), sent(M, N, dtype=torch.bfloat16)
        torch.cuda.synchronize()
        ctx.check(ctx.lib.rt_debug_reduce_slabs(ctx.handle, P(sd), n_slabs, M, N, P(b), 0, P(o32) if want32 else None, P(obf) if wantbf else None),
                  "rt_debug_reduce_slabs")
        want = ref if b is not None else R.reduce_slabs_ref(slabs).float()
        R.check_bits(o32.cpu(), want if want32 else sent(M, N).cpu(), f"f32 {want32} {wantbf}")
        R.check_bits(obf.cpu(), R.bf16(want) if wantbf else sent(M, N, dtype=torch.bfloat16).cpu(), f"bf16 {want32} {wantbf}")
    rs = randn(n_slabs, M, N, seed=3)
    rd = dev(rs)
    for act in (R.ACT_SILU, R.ACT_GELU):
        o32 = sent(M, N)
        torch.cuda.synchronize()
        ctx.check(ctx.lib.rt_debug_reduce_slabs(ctx.handle, P(rd), n_slabs, M, N, P(bd), act, P(o32), None), "rt_debug_reduce_slabs")
        R.check_rel(o32.cpu(), R.reduce_slabs_ref(rs, bias, act), 1e-5, f"act {act}", floor=1.0)


def test_f32_to_bf16_rounding_and_special_values(ctx):
    """Ties to even both ways, +-0, +-inf, NaN stays NaN (a NaN whose payload sits in the dropped bits included), the largest
    finite float (rounds to infinity), and a tensor past the grid cap (8192 x 256 + 3001 elements) against the CPU's rounding."""
    pats = [0x3F808000, 0x3F818000, 0x3F808001, 0x3F817FFF, 0xBF808000, 0xBF818000, 0x00000000, 0x80000000, 0x7F800000, 0xFF800000,
            0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F7FFF, 0x7FC00000, 0x7F800001, 0xFFC12345]
    want = [0x3F80, 0x3F82, 0x3F81, 0x3F81, 0xBF80, 0xBF82, 0x0000, 0x8000, 0x7F80, 0xFF80, 0x7F80, 0xFF80, 0x7F7F]
    xd = torch.tensor([p - (1 << 32) if p >= (1 << 31) else p for p in pats], dtype=torch.int32).view(torch.float32).cuda()
    out = sent(len(pats), dtype=torch.bfloat16)
    torch.cuda.synchronize()
    ctx.check(ctx.lib.rt_debug_f32_to_bf16(ctx.handle, P(xd), len(pats), P(out)), "rt_debug_f32_to_bf16")
    got = [int(v) & 0xFFFF for v in out.cpu().view(torch.int16).tolist()]
    assert got[:len(want)] == want, [hex(g) for g in got]
    for g in got[len(want):]:                                   # NaN stays NaN
        assert (g & 0x7F80) == 0x7F80 and (g & 0x7F) != 0, hex(g)
    n = 8192 * 256 + 3001
    big = randn(n, seed=1)
    bd, out = big.cuda(), sent(n + 8, dtype=torch.bfloat16)
    torch.cuda.synchronize()
    ctx.check(ctx.lib.rt_debug_f32_to_bf16(ctx.handle, P(bd), n, P(out)), "rt_debug_f32_to_bf16")
    R.check_bits(out.cpu()[:n], R.bf16(big), "past the grid cap")
    R.check_bits(out.cpu()[n:], torch.full((8,), SENT, dtype=torch.bfloat16), "guard")


# ================================================================================================ 6. k_qkv_post
@pytest.mark.parametrize("lo_planes", [False, True])
@pytest.mark.parametrize("rope", [True, False])
@pytest.mark.parametrize("norm", [True, False])
@pytest.mark.parametrize("n_slabs", [1, 3])
@pytest.mark.parametrize("heads,kv,d", [(3, 1, 2), (4, 2, 32), (2, 2, 64), (4, 2, 128)])
def test_qkv_post(ctx, heads, kv, d, n_slabs, norm, rope, lo_planes):
    """k_qkv_post: head_dim 2 .. 128 (below 128 lanes are inactive), positions 0 and max_pos - 1 (with pos_add = 3 and frame = 2
    on top of row_pos), distinct slots.  q against float64 at 1e-5 * max|ref|; cache rows at bf16's half ulp 2^-8 |ref| (plus the
    float32 error) without low planes, 2^-16 |ref| with them; every cache element no row addresses keeps its bit pattern."""
    M, slots, max_pos, pos_add, frame = 5, 6, 16, 3, 2
    width = (heads + 2 * kv) * d
    slabs = randn(n_slabs, M, width, seed=1)
    qw, kw = (1 + 0.1 * randn(d, seed=2), 1 + 0.1 * randn(d, seed=3)) if norm else (None, None)
    ang = randn(max_pos, d // 2, seed=4)
    cos, sin = (torch.cos(ang), torch.sin(ang)) if rope else (None, None)
    row_slot = [4, 0, 5, 2, 2]
    pos = [0, max_pos - 1, 7, 3, 4]                              # (slot 2 takes two rows at different positions)
    row_pos = [p - pos_add - frame for p in pos]
    keep = [dev(slabs), dev(qw), dev(kw), dev(cos), dev(sin), i32(row_slot), i32(row_pos), i32([frame])]
    q_out = sent(M, heads, d)
    caches = [sent(slots, kv, max_pos, d, dtype=torch.bfloat16) for _ in range(4)]
    torch.cuda.synchronize()
    rc = ctx.lib.rt_debug_qkv_post(ctx.handle, P(keep[0]), n_slabs, M, heads, kv, d, P(keep[1]), P(keep[2]), EPS, P(keep[3]), P(keep[4]), P(keep[5]),
                                   P(keep[6]), pos_add, P(q_out), P(caches[0]), P(caches[1]), P(caches[2]) if lo_planes else None,
                                   P(caches[3]) if lo_planes else None, slots, max_pos, P(keep[7]))
    ctx.check(rc, "rt_debug_qkv_post")
    q_ref, k_ref, v_ref = R.qkv_post_ref(slabs, heads, kv, d, qw, kw, EPS, cos, sin, torch.tensor(pos))
    R.check_rel(q_out.cpu(), q_ref, 1e-5, "q")
    written = torch.zeros(slots, kv, max_pos, d, dtype=torch.bool)
    for s, p in zip(row_slot, pos):
        written[s, :, p, :] = True
    for name, hi, lo, ref in (("k", caches[0], caches[2], k_ref), ("v", caches[1], caches[3], v_ref)):
        hi, lo = hi.cpu(), lo.cpu()
        rows = torch.stack([hi[s, :, p, :] for s, p in zip(row_slot, pos)]).float().to(F64)
        floor = 1e-5 * float(ref.abs().max())
        R.check_untouched(hi, SENT, written, name + " cache")
        if lo_planes:
            lrows = torch.stack([lo[s, :, p, :] for s, p in zip(row_slot, pos)]).float().to(F64)
            R.check_close(rows + lrows, ref, 2.0 ** -16 * ref.abs() + floor, name + " hi + lo")
            R.check_close(rows, ref, 2.0 ** -8 * ref.abs() + floor, name + " hi")
            R.check_untouched(lo, SENT, written, name + " low plane")
        else:
            R.check_close(rows, ref, 2.0 ** -8 * ref.abs() + floor, name)
            R.check_bits(lo, sent(slots, kv, max_pos, d, dtype=torch.bfloat16).cpu(), name + " low plane not given: untouched")


def test_qkv_post_refusals(ctx):
    M, heads, kv = 2, 2, 1
    for d, slot, pos in ((130, 0, 0), (3, 0, 0), (32, 9, 0), (32, 0, 16)):
        width = (heads + 2 * kv) * d
        keep = [dev(randn(1, M, width, seed=1)), i32([slot, 0]), i32([pos, 0])]
        q_out = sent(M, heads, d)
        caches = [sent(2, kv, 16, d, dtype=torch.bfloat16) for _ in range(2)]
        torch.cuda.synchronize()
        rc = ctx.lib.rt_debug_qkv_post(ctx.handle, P(keep[0]), 1, M, heads, kv, d, None, None, EPS, None, None, P(keep[1]), P(keep[2]), 0, P(q_out),
                                       P(caches[0]), P(caches[1]), None, None, 2, 16, None)
        refused(ctx, rc, f"d={d} slot={slot} pos={pos}")
        R.check_bits(q_out.cpu(), sent(M, heads, d).cpu())


# ================================================================================================ 7. gathers, code embedding, depthwise conv
@pytest.mark.parametrize("H", [1, 300])
def test_gather_sum_and_gather_f32(ctx, H):
    """k_gather_sum / k_gather_f32 with integer-valued tables: bit-exact; H = 300 gives 44 lanes a second element; index stride
    above n_src, the index array at frame 2, add_rows through a negative add_row_idx, negative indices."""
    M, V, n_src, stride, frame = 6, 7, 3, 5, 2
    fs = M * stride + 1
    tabs = [R.bf16(randint(-3, 3, V, H + 2, seed=10 + j)) for j in range(n_src)]
    add_vec, add_rows = randint(-3, 3, H, seed=20), randint(-3, 3, M, H, seed=21)
    add_row_idx = [3, -1, 0, 2, -5, 1]
    idx = torch.randint(0, V, (3, fs), generator=gen(22), dtype=torch.int32)
    idx[torch.rand(3, fs, generator=gen(23)) < 0.3] = -1
    idx[2, 0], idx[2, 1] = 2, -1
    td, ivd, ard, arid, idd, fd = [dev(t) for t in tabs], dev(add_vec), dev(add_rows), i32(add_row_idx), dev(idx), i32([frame])
    tp, sp = tables_arg(td, [H + 2] * n_src)
    rows = idx[frame, :M * stride].reshape(M, stride).long()
    for use_vec, use_rows, use_map in ((True, True, True), (False, False, False), (True, True, False), (False, True, True)):
        ar_t, ref_rows, ref_map = ard, add_rows, torch.tensor(add_row_idx)
        o32, obf = sent(M, H), sent(M, H, dtype=torch.bfloat16)
        torch.cuda.synchronize()
        rc = ctx.lib.rt_debug_gather_sum(ctx.handle, tp, sp, n_src, P(idd), M, H, P(ivd) if use_vec else None, P(ar_t) if use_rows else None,
                                         P(arid) if (use_rows and use_map) else None, P(o32), P(obf), stride, P(fd), fs)
        ctx.check(rc, "rt_debug_gather_sum")
        ref, _ = R.embed_ref([t[:, :H] for t in tabs], rows, add_vec if use_vec else None, None, ref_rows if use_rows else None,
                             ref_map if (use_rows and use_map) else None)
        R.check_bits(o32.cpu(), ref.float(), f"gather_sum H={H} vec={use_vec} rows={use_rows} map={use_map}")
        R.check_bits(obf.cpu(), R.bf16(ref.float()), "gather_sum bf16")
    # default index stride (0 = n_src), no frame pointer, one output
    idx0 = dev(idx[0, :M * n_src].contiguous())
    o32 = sent(M, H)
    torch.cuda.synchronize()
    ctx.check(ctx.lib.rt_debug_gather_sum(ctx.handle, tp, sp, n_src, P(idx0), M, H, None, None, None, P(o32), None, 0, None, 0), "rt_debug_gather_sum")
    ref, _ = R.embed_ref([t[:, :H] for t in tabs], idx[0, :M * n_src].reshape(M, n_src).long())
    R.check_bits(o32.cpu(), ref.float(), "gather_sum default stride")
    # k_gather_f32
    table = randn(V, H, seed=25)
    tbd = dev(table)
    o32, obf = sent(M, H), sent(M, H, dtype=torch.bfloat16)
    torch.cuda.synchronize()
    ctx.check(ctx.lib.rt_debug_gather_f32(ctx.handle, P(tbd), H, P(idd), M, P(o32), P(obf), stride, P(fd), fs), "rt_debug_gather_f32")
    ref = R.gather_rows_ref(table, rows[:, 0]).float()
    R.check_bits(o32.cpu(), ref, f"gather_f32 H={H}")
    R.check_bits(obf.cpu(), R.bf16(ref), "gather_f32 bf16")
    assert bool((rows[:, 0] < 0).any()), "the case holds a negative index"


@pytest.mark.parametrize("Q", [1, 16])
@pytest.mark.parametrize("H", [1, 300])
def test_code_embed_mean(ctx, H, Q):
    """k_code_embed_mean: codes below 0 and at or above the codebook size clamp; integer tables and a power-of-two Q: bit-exact."""
    rows, cb = 7, 5
    table = R.bf16(randint(-3, 3, Q, cb, H, seed=1))
    codes = torch.randint(-2, cb + 3, (rows, Q), generator=gen(2), dtype=torch.int32)
    codes[0, 0], codes[1, 0], codes[2, 0] = -1, cb, cb + 100
    td, cd, out = dev(table), dev(codes), sent(rows, H)
    torch.cuda.synchronize()
    ctx.check(ctx.lib.rt_debug_code_embed_mean(ctx.handle, P(td), cb, Q, H, P(cd), rows, P(out)), "rt_debug_code_embed_mean")
    R.check_bits(out.cpu(), R.code_embed_mean_ref(table.float(), codes).float(), f"H={H} Q={Q}")


@pytest.mark.parametrize("T", [1, 5, 8])
@pytest.mark.parametrize("C", [1, 300, 1024])
def test_dwconv_ln(ctx, C, T):
    """k_dwconv_ln, B = 2: the first six rows of item 1 must not see item 0 (the input makes a leak visible far above the tolerance:
    tests/test_rowops_ref_cpu.py).  float64 at 1e-5 * max|ref|; C = 1 has variance 0, so the output is ln_b to 1e-6."""
    x, w, b, lw, lb = R.dwconv_case(C, T)
    keep = [dev(t) for t in (x, w, b, lw, lb)]
    out = sent(2, T, C)
    torch.cuda.synchronize()
    ctx.check(ctx.lib.rt_debug_dwconv_ln(ctx.handle, P(keep[0]), 2, T, C, P(keep[1]), P(keep[2]), P(keep[3]), P(keep[4]), 1e-5, P(out)),
              "rt_debug_dwconv_ln")
    if C == 1:
        R.check_close(out.cpu(), lb.expand(2, T, 1), 1e-6, "C = 1")
    else:
        R.check_rel(out.cpu(), R.dwconv_ln_ref(x, w, b, lw, lb, 1e-5), 1e-5, f"C={C} T={T}")


# ================================================================================================ 8. k_final_conv
def final_conv(ctx, x, w, bias, wav_stride):
    B, T, Cc = x.shape
    hi, lo = R.planes(x)
    keep = [dev(hi), dev(lo), dev(w), dev(bias)]
    wav = sent(B, max(wav_stride, 1))
    torch.cuda.synchronize()
    rc = ctx.lib.rt_debug_final_conv(ctx.handle, P(keep[0]), P(keep[1]), B, T, Cc, P(keep[2]), P(keep[3]), P(wav), wav_stride)
    return rc, wav.cpu(), hi.float().to(F64) + lo.float().to(F64)


@pytest.mark.parametrize("T", [1, 127, 128, 129, 300])
@pytest.mark.parametrize("C", [16, 96, 112])
def test_final_conv(ctx, C, T):
    """k_final_conv: C = 112 needs a second round of the window loader (134 * 14 = 1876 > 1792 requests), T around the 128-sample
    workgroup; wav_stride = T + 5 with the five elements behind every row untouched.  Integer planes, weights and bias times one
    power of two: exact, some samples saturated at +-1 and others strictly inside (asserted on the CPU for T = 300), so bit-exact.
    Random operands: float64 of the planes' sum at 1e-5 * max(1, sum|terms|)."""
    stride = T + 5
    written = torch.zeros(2, stride, dtype=torch.bool)
    written[:, :T] = True
    x, w, bias = R.final_conv_int_case(C, T)
    rc, wav, xs = final_conv(ctx, x, w, bias, stride)
    ctx.check(rc, "rt_debug_final_conv")
    assert torch.equal(xs, x.to(F64))
    yc, y, _ = R.final_conv_ref(x, w, bias)
    R.check_bits(wav[:, :T], yc.float(), f"integer form C={C} T={T}")
    R.check_untouched(wav, SENT, written, "behind the rows")
    x, w, bias = randn(2, T, C, seed=1), 0.05 * randn(7, C, seed=2), 0.1 * randn(1, seed=3)
    rc, wav, xs = final_conv(ctx, x, w, bias, stride)
    ctx.check(rc, "rt_debug_final_conv")
    yc, y, mag = R.final_conv_ref(xs, w, bias)
    R.check_close(wav[:, :T], yc, 1e-5 * mag.clamp(min=1.0), f"random form C={C} T={T}")
    R.check_untouched(wav, SENT, written, "behind the rows")


@pytest.mark.parametrize("C,T,stride", [(120, 10, 15), (24, 10, 15), (96, 10, 9)])
def test_final_conv_refusals(ctx, C, T, stride):
    rc, wav, _ = final_conv(ctx, randn(2, T, C, seed=1), randn(7, C, seed=2), randn(1, seed=3), stride)
    refused(ctx, rc, f"C={C} wav_stride={stride}")
    R.check_bits(wav, sent(2, stride).cpu())
