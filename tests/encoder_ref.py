"""References of the conditioning front-end's own kernels (rho_tts_amd/csrc/encoder.hip: k_enc_conv0, k_rvq, k_stats_pool,
k_gemv_f32) and of its stages (voice.hip voice_encode_impl), with the inputs the CPU and the GPU tests share.

Plain numpy / torch in float64; where the kernel's float32 evaluation order is DEFINED (encoder.hip is built without
contraction), a float32 mirror of that order, whose bits a correct kernel must reproduce.  Everything here runs on the CPU;
tests/test_encoder_ref_cpu.py holds the references to oracle/encoder.py and shows that every comparison of
tests/test_encoder_kernels_gpu.py rejects a reference with one minimal defect (the keyword arguments named `defect`).

Tolerances live here, next to the arithmetic they bound, each with its derivation; u = 2^-24 is the unit roundoff of float32."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle import encoder as E

F64 = torch.float64
U24 = 2.0 ** -24
# A float32 value read as hi + lo bf16 planes keeps 16 significand bits: hi = bf16(v) is off by <= 2^-9 |v|, lo = bf16(v - hi) by
# <= 2^-9 |v - hi| <= 2^-18 |v|.  2^-17 bounds that with the second-order terms.
PLANES_REL = 2.0 ** -17
# HIP's expm1f is documented at 1 ulp (ROCm "HIP math API", single precision table): 2^-23 relative; 2^-22 with the rounding of the
# float64 reference to float32 on top.
EXPM1F_REL = 2.0 ** -22


# ------------------------------------------------------------------------------------------ k_enc_conv0
def conv0_ref(pcm, w, bias, mirror=False, defect=None):
    """x[t][c] = bias[c] + sum_k w[c][k] * pcm[t - (K - 1) + k], zeros in front of the clip.  pcm [T], w [C][K], bias [C] float32
    arrays -> [T][C] float64; mirror=True: float32 in the kernel's order (bias first, taps ascending, separate multiply and add,
    a tap in front of the clip adds nothing).  defect "leak": the first K - 1 outputs read pcm[0] instead of zero."""
    pcm, w, bias = (np.asarray(a, dtype=np.float32) for a in (pcm, w, bias))
    T, (C, K) = pcm.shape[0], w.shape
    dt = np.float32 if mirror else np.float64
    acc = np.broadcast_to(bias.astype(dt), (T, C)).copy()
    t = np.arange(T)
    for k in range(K):
        ti = t - (K - 1) + k
        valid = ti >= 0
        p = pcm[np.maximum(ti, 0)].astype(dt)
        if defect == "leak":
            valid = np.ones_like(valid)
        term = (w[:, k].astype(dt)[None, :] * p[:, None]).astype(dt)
        acc = np.where(valid[:, None], (acc + term).astype(dt), acc)
    return acc


def elu_planes_ref(x, defect=None):
    """The kernel's second output: e = x > 0 ? x : expm1f(x), hi = bf16(e), lo = bf16(e - hi).  x: the kernel's OWN float32 x.
    Returns (hi, lo, e64): hi / lo as computed from the CPU's float32 ELU - the bits a correct kernel produces wherever x >= 0
    (e = x there, expm1f(+-0) = +-0, no library involved) - and e64 = the float64 ELU, for elu_neg_tol where x < 0.
    defect "lo0": a lo plane of zeros."""
    x = torch.as_tensor(x, dtype=torch.float32)
    e32 = torch.where(x > 0, x, torch.expm1(x))
    hi = e32.to(torch.bfloat16)
    lo = (e32 - hi.float()).to(torch.bfloat16)
    if defect == "lo0":
        lo = torch.zeros_like(lo)
    x64 = x.to(F64)
    return hi, lo, torch.where(x64 > 0, x64, torch.expm1(x64))


def elu_neg_tol(e64):
    """Bound on |hi + lo - ELU(x)| where x < 0: the two planes keep 16 significand bits of the kernel's float32 e (PLANES_REL), and
    e = expm1f(x) itself is within 1 ulp of the true value (EXPM1F_REL).  Nothing measured enters."""
    return (PLANES_REL + EXPM1F_REL) * e64.abs()


# ------------------------------------------------------------------------------------------ k_rvq
def rvq_distances(x, cb, order="asc", fma=False, f64=False, drop_last_dim=False):
    """d[t][j] = sum_k (x[t][k] - cb[j][k])^2.  The DEFINED evaluation (oracle.encoder.rvq_level, k_rvq): float32, ascending k, the
    difference, the product and the sum each rounded once.  The other arguments are wrong evaluations a kernel could fall into:
    descending k; a fused multiply-add (the product unrounded: exact in float64, the sum then rounded to float32 once - float64
    itself rounds the sum in the rare case it needs more than 53 bits, which makes this no less wrong); float64 throughout; the
    last dimension left out."""
    x, cb = np.asarray(x, dtype=np.float32), np.asarray(cb, dtype=np.float32)
    T, D = x.shape
    ks = list(range(D - 1 if drop_last_dim else D))
    if order == "desc":
        ks = ks[::-1]
    if f64:
        acc = np.zeros((T, cb.shape[0]), dtype=np.float64)
        for k in ks:
            diff = x[:, k:k + 1].astype(np.float64) - cb[None, :, k].astype(np.float64)
            acc += diff * diff
        return acc
    acc = np.zeros((T, cb.shape[0]), dtype=np.float32)
    for k in ks:
        diff = (x[:, k:k + 1] - cb[None, :, k]).astype(np.float32)
        if fma:
            acc = (acc.astype(np.float64) + diff.astype(np.float64) * diff.astype(np.float64)).astype(np.float32)
        else:
            acc = (acc + (diff * diff).astype(np.float32)).astype(np.float32)
    return acc


def rvq_level_ref(x, cb, defect=None, **evaluation):
    """Nearest entry per row, the lowest index on equal distances.  defects: "highest" (the highest index wins a tie), "no_last_dim",
    "no_last_entry" (entry K - 1 is never considered)."""
    d = rvq_distances(x, cb, drop_last_dim=defect == "no_last_dim", **evaluation)
    if defect == "no_last_entry":
        d = d[:, :-1]
    if defect == "highest":
        return d.shape[1] - 1 - d[:, ::-1].argmin(axis=1)
    return d.argmin(axis=1)


def rvq_ref(sem, aco, cbs, defect=None):
    """The split residual quantiser as rt_debug_rvq states it: cbs = Q codebooks [K][D] float32; level 0 quantises sem, levels
    1 .. Q - 1 quantise aco residually (float32 subtraction of the chosen entry).  Returns (codes [T][Q] int64, the residual after
    the last level [T][D] float32 - aco itself when Q == 1).  defect "wrong_level": the residual is taken from the codebook of the
    level before; the level defects of rvq_level_ref apply to every level."""
    sem, res = np.asarray(sem, dtype=np.float32), np.asarray(aco, dtype=np.float32).copy()
    Q = len(cbs)
    codes = np.zeros((sem.shape[0], Q), dtype=np.int64)
    lv = None if defect == "wrong_level" else defect
    codes[:, 0] = rvq_level_ref(sem, cbs[0], lv)
    for q in range(1, Q):
        cb = np.asarray(cbs[q], dtype=np.float32)
        idx = rvq_level_ref(res, cb, lv)
        codes[:, q] = idx
        sub = np.asarray(cbs[q - 1], dtype=np.float32) if defect == "wrong_level" else cb
        res = (res - sub[idx]).astype(np.float32)
    return codes, res


# ------------------------------------------------------------------------------------------ k_stats_pool
def stats_pool_ref(x, defect=None):
    """x [T][C] -> [2 C] float64: the mean over t, then sqrt(variance about that mean + 1e-5).  defect "about_zero": the variance
    taken about 0."""
    x = torch.as_tensor(x).to(F64)
    mean = x.mean(0)
    d = x if defect == "about_zero" else x - mean
    return torch.cat([mean, torch.sqrt((d * d).mean(0) + 1e-5)])


def stats_pool_mirror(x):
    """float32 in the kernel's order: four time lanes (t = lane, lane + 4, ...) summed serially, the four partial sums added
    left to right, a division by T; the same again for the squared deviations (difference, product and sum each rounded), then
    + 1e-5 and the square root."""
    x = np.asarray(x, dtype=np.float32)
    T, C = x.shape

    def lanes(v):
        part = []
        for lane in range(4):
            s = np.zeros(C, dtype=np.float32)
            for t in range(lane, T, 4):
                s = (s + v[t]).astype(np.float32)
            part.append(s)
        return (((part[0] + part[1]).astype(np.float32) + part[2]).astype(np.float32) + part[3]).astype(np.float32)
    mean = (lanes(x) / np.float32(T)).astype(np.float32)
    d = (x - mean[None, :]).astype(np.float32)
    var = (lanes((d * d).astype(np.float32)) / np.float32(T)).astype(np.float32)
    return np.concatenate([mean, np.sqrt((var + np.float32(1e-5)).astype(np.float32)).astype(np.float32)])


def stats_pool_tol(x):
    """Element-wise bounds (mean [C], deviation [C]) on the kernel's float32 result against stats_pool_ref, from T alone.
    A lane adds ceil(T / 4) terms, three more adds join the lanes and one division follows: n = ceil(T / 4) + 4 roundings, each at
    most u times the running magnitude <= sum |x|:  |dmean| <= n u sum|x| / T.
    Deviations d = x - mean: the shift dmean of the mean drops out of sum d^2 to first order (sum d = 0) and leaves T dmean^2;
    rounding d and d * d costs 2 u per term, the sums and the division n u:  |dV| <= (n + 2) u V + dmean^2, V = sum d^2 / T.
    s = sqrt(V + 1e-5): |ds| <= |dV| / (2 s) + 2 u s (the addition and the square root)."""
    x = torch.as_tensor(x).to(F64)
    T = x.shape[0]
    n = math.ceil(T / 4) + 4
    dmean = n * U24 * x.abs().sum(0) / T
    mean = x.mean(0)
    V = ((x - mean) ** 2).mean(0)
    s = torch.sqrt(V + 1e-5)
    return dmean, ((n + 2) * U24 * V + dmean ** 2) / (2 * s) + 2 * U24 * s


def ulps_apart(a, b):
    """Distance in float32 ulps between two float32 arrays of one sign pattern (the deviations: positive)."""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


# ------------------------------------------------------------------------------------------ k_gemv_f32
def gemv_ref(W, b, x, relu, defect=None):
    """y = W x + b, max(y, 0) when relu.  Returns (y [N] float64, mag [N] = sum_k |w||x| + |b|, the magnitude the rounding bound
    (K + 1) u mag scales with: K products and K adds in some order, the bias as one more term of the sum).  defect "no_last_row":
    row N - 1 is not computed (stays 0)."""
    W, x = torch.as_tensor(W).to(F64), torch.as_tensor(x).to(F64)
    y, mag = W @ x, W.abs() @ x.abs()
    if b is not None:
        y, mag = y + torch.as_tensor(b).to(F64), mag + torch.as_tensor(b).to(F64).abs()
    if relu:
        y = y.clamp(min=0)
    if defect == "no_last_row":
        y = y.clone()
        y[-1] = 0
    return y, mag


# ------------------------------------------------------------------------------------------ comparison
def assert_equal(got, want, what=""):
    """Exact equality of two integer or float arrays, NaN-free (codes, residuals, float32 mirrors); compared as bit patterns."""
    g, w = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert g.shape == w.shape and g.dtype == w.dtype, (what, g.shape, w.shape, g.dtype, w.dtype)
    gb, wb = (a.view({2: np.int16, 4: np.int32, 8: np.int64}[a.itemsize]) for a in (g, w))
    bad = gb != wb
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} elements differ, first at {tuple(np.argwhere(bad)[0])}"


# ------------------------------------------------------------------------------------------ inputs of the quantiser tests
def _rng(seed):
    return np.random.default_rng(seed)


def rvq_tie_positions(K):
    """Pairs (or singletons) of codebook positions where an exact duplicate of the winner is planted, one pattern per frame in turn:
    two entries of one thread (j, j + 1024, ...), two lanes of one wave, two waves, index 0, index K - 1 (alone: it must be considered; and behind a lower duplicate), the last,
    partly filled wave.  Positions outside [0, K) are dropped."""
    last_wave = (K - 1) // 64 * 64
    pats = [(5, 5 + 1024), (70, 70 + 2048), (9, 9 + 3072), (130, 137), (3, 3 + 64 * 3), (0, K // 2), (K - 1,), (K - 1, K // 3), (last_wave, K - 1),
            (last_wave + (K - 1 - last_wave) // 2, 1), (1024, 2047), (2048 + 17, 1024 + 17)]
    out = []
    for p in pats:
        q = tuple(sorted({v for v in p if 0 <= v < K}))
        if q:
            out.append(q)
    return out


def rvq_int_case(T, D, K, Q, seed):
    """Integer-valued vectors and codebooks (vectors |v| <= 2, entries |c| <= 3 or a planted vector, so residuals stay within
    2 + 3 Q and every distance is an integer <= (5 + 6 Q)^2 D < 2^24 for Q <= 5, D <= 4096: exact in float32 in any order),
    with exact duplicates of an entry one unit from each frame's vector planted level by level at rvq_tie_positions - so the
    winner is decided by the index rule alone.  Returns (sem, aco, cbs, planted) with planted[q][t] = the positions planted for
    frame t at level q."""
    g = _rng(seed)
    sem = g.integers(-2, 3, (T, D)).astype(np.float32)
    aco = g.integers(-2, 3, (T, D)).astype(np.float32)
    cbs, planted = [], []
    pats = rvq_tie_positions(K)
    res = aco.copy()
    for q in range(Q):
        cb = g.integers(-3, 4, (K, D)).astype(np.float32)
        x = sem if q == 0 else res
        pl, used = [], set()
        for t in range(T):
            # the pattern of this frame, moved along (upwards, or downwards from the codebook's end) until its positions are free:
            # frames that share a pattern keep its kind - the same thread, the same wave - at other positions
            base, sh, pos = pats[(t + q) % len(pats)], 11 * ((t + q) // len(pats)), ()
            for sh in range(sh, sh + K):
                cand = tuple(sorted({v + sh if v + sh < K else v - sh for v in base}))
                if len(cand) == len(base) and cand[0] >= 0 and not used & set(cand):
                    pos = cand
                    break
            used |= set(pos)
            if pos:
                near = x[t].copy()
                # one unit off in two random dimensions (one when D == 1): the same small distance at every planted position, and
                # the residual of the level is those units - not zero, and rarely the same for two frames
                near[g.choice(D, min(2, D), replace=False)] += g.choice([-1.0, 1.0], min(2, D))
                cb[list(pos)] = near
            pl.append(pos)                             # (empty: the codebook is too small for another frame's pair)
        cbs.append(cb)
        planted.append(pl)
        if q >= 1:
            res = (res - cb[rvq_level_ref(res, cb)]).astype(np.float32)
    return sem, aco, cbs, planted


def rvq_census_case(T, D, K, Q, seed):
    """A planted census: every codebook row is its own index written in base b over the first nd = min(D, 4) dimensions (distinct
    rows at least one unit apart), level q >= 1 scaled by 2^-(s (q - 1)); sem[t] = cb_0[target[t][0]], aco[t] = sum over q >= 1 of
    cb_q[target[t][q]].  s is chosen so that everything behind level q is shorter than a quarter of that level's unit
    (2^s > 4 sqrt(nd) (b - 1) / (1 - 2^-s)): the target is then at most a quarter unit away and every other entry at least three
    quarters - a margin no float32 rounding closes.  The sums and the residuals are exact in float32 (asserted here).  Returns
    (sem, aco, cbs, target [T][Q])."""
    g = _rng(seed)
    nd = min(D, 4)
    b = max(2, math.ceil(K ** (1.0 / nd) - 1e-9))
    while b ** nd < K:
        b += 1
    s = 1
    while 2.0 ** s * (1 - 2.0 ** -s) <= 4 * math.sqrt(nd) * (b - 1):
        s += 1
    cbs = []
    for q in range(Q):
        idx = g.permutation(K)
        rows = np.zeros((K, D), dtype=np.float64)
        for i in range(nd):
            rows[:, i] = (idx // b ** i) % b
        cbs.append(rows * (2.0 ** (-s * max(q - 1, 0))))
    target = g.integers(0, K, (T, Q))
    target[0, :] = 0
    target[-1, :] = K - 1
    sem = cbs[0][target[:, 0]]
    aco = np.zeros((T, D))
    for q in range(1, Q):
        aco = aco + cbs[q][target[:, q]]
    for a in [sem, aco] + cbs:
        assert np.array_equal(a.astype(np.float32).astype(np.float64), a), "census case does not fit float32: fewer levels or a smaller K"
    return sem.astype(np.float32), aco.astype(np.float32), [c.astype(np.float32) for c in cbs], target


def rvq_near_tie_case(T, D, K, cluster, seed):
    """An input on which the EVALUATION ORDER decides the code.  For every frame a cluster of `cluster` entries is planted around
    x[t], equidistant from it up to rounding: a base entry x + r reflected about x in random coordinates (x - r there), then random
    coordinates nudged by one float32 ulp.  All other entries are clearly farther.  Returns (x [T][D], cb [K][D]) float32."""
    g = _rng(seed)
    x = g.standard_normal((T, D)).astype(np.float32)
    cb = (3.0 * g.standard_normal((K, D))).astype(np.float32)
    slots = g.permutation(K)[:T * cluster].reshape(T, cluster)
    for t in range(T):
        r = (0.2 + 0.3 * g.random(D)).astype(np.float32) * g.choice([-1.0, 1.0], D).astype(np.float32)
        for j in range(cluster):
            sign = np.where(g.random(D) < 0.5, -1.0, 1.0).astype(np.float32)
            c = (x[t] + sign * r).astype(np.float32)
            nudge = g.random(D) < 0.25
            c = np.where(nudge, np.nextafter(c, np.where(g.random(D) < 0.5, -np.inf, np.inf).astype(np.float32)), c).astype(np.float32)
            cb[slots[t, j]] = c
    return x, cb


NEAR_TIE = dict(T=33, D=40, K=1100, cluster=8, seed=5)          # the shared near-tie input (flip counts: tests/test_encoder_ref_cpu.py)
NEAR_TIE_2 = dict(T=64, D=24, K=2049, cluster=8, seed=5)


# ------------------------------------------------------------------------------------------ stages of voice_encode_impl
class Bounded:
    """A float64 activation [1][C][T] and an element-wise bound on the GPU's error on it."""

    def __init__(self, v, err=None):
        self.v, self.err = v, torch.zeros_like(v) if err is None else err


def _conv_bounded(a, w, b, stride=1, pad_mode="constant", operand_rel=PLANES_REL):
    """A causal conv of the reference a.v, and the propagated bound: the operand the GPU multiplies is off by a.err plus
    operand_rel |a| (it is read as hi + lo bf16 planes), every product is exact (bf16 x bf16 in float32), the matrix cores add
    2 K products (two planes, K = taps x channels) and the bias in float32: (2 K + 2) u (|w| * |a| + |b|)."""
    w64 = w.to(F64)
    Kred = w.shape[1] * w.shape[2]
    v = E.causal_conv(a.v, w64, None if b is None else b.to(F64), stride=stride, pad_mode=pad_mode)
    mag = E.causal_conv(a.v.abs() + a.err, w64.abs(), None if b is None else b.to(F64).abs(), stride=stride, pad_mode=pad_mode)
    op = E.causal_conv(a.err + operand_rel * (a.v.abs() + a.err), w64.abs(), None, stride=stride, pad_mode=pad_mode)
    return Bounded(v, op + (2 * Kred + 2) * U24 * mag)


def seanet_ref(W, cfg, pcm):
    """oracle.encoder.seanet_encode chained in float64 on the clip -> (feats [Te][He] float64, bound), bound(flat indices) = the
    derived bound on the GPU's error at those elements of feats.

    Every place where the GPU's arithmetic departs from the exact chain is a point where an error e with |e| <= b (element-wise)
    enters:
      the first conv, float32 on exact operands:        b = (K + 1) u (|w| * |pcm| + |bias|)
      every later conv's operand ELU(x) as two planes:  b = PLANES_REL |ELU(x)|, + EXPM1F_REL |ELU(x)| where x < 0 (expm1f)
      every later conv's sums on the matrix cores:      b = (2 K + 2) u (|w| * |ELU(x)| + |bias|)   (two planes of K = taps x channels
                                                        exact products each, the bias, the store)
      every residual add:                               b = u |x + y|
    To first order the error of output o is sum over points and elements of d o / d e . e, so |error_o| <= sum |d o / d e| b: the
    Jacobians come from autograd on the float64 chain (the errors are zeros added at those points), with their signs and
    cancellations - a product of |w| through all layers instead would exceed the signal itself.  Second-order terms are
    2^-17 of the first-order ones.  A Jacobian row per output element costs a backward pass, so the bound is evaluated where
    the caller asks."""
    c = cfg.codec
    zs, bs = [], []

    def inject(v, b):
        z = torch.zeros_like(v, requires_grad=True)
        zs.append(z)
        bs.append(b.detach())
        return v + z

    def conv(x, i, stride=1):
        w, b = W[f"enc.conv.{i}.weight"].to(F64), W[f"enc.conv.{i}.bias"].to(F64)
        e = F.elu(x)
        rel = PLANES_REL + EXPM1F_REL * (x.detach() < 0).to(F64)
        o = inject(e, rel * e.detach().abs())
        y = E.causal_conv(o, w, b, stride=stride)
        mag = E.causal_conv(e.detach().abs(), w.abs(), b.abs(), stride=stride)
        return inject(y, (2 * w.shape[1] * w.shape[2] + 2) * U24 * mag)

    h = torch.as_tensor(np.asarray(pcm, dtype=np.float32)).to(F64).reshape(1, 1, -1)
    w0, b0 = W["enc.conv.0.weight"].to(F64), W["enc.conv.0.bias"].to(F64)
    x = inject(E.causal_conv(h, w0, b0), (w0.shape[-1] + 1) * U24 * E.causal_conv(h.abs(), w0.abs(), b0.abs()))
    i = 1
    for r in c.enc_ratios:
        s = x + conv(conv(x, i), i + 1)
        x = conv(inject(s, U24 * s.detach().abs()), i + 2, stride=r)
        i += 3
    feats = conv(x, i)[0].T                                         # [Te][He]

    def bound(flat_idx, batch=64):
        out = []
        for chunk in torch.as_tensor(flat_idx, dtype=torch.long).split(batch):
            go = torch.zeros(len(chunk), feats.numel(), dtype=F64)
            go[torch.arange(len(chunk)), chunk] = 1.0
            grads = torch.autograd.grad(feats, zs, grad_outputs=go.reshape(len(chunk), *feats.shape), is_grads_batched=True, retain_graph=True)
            out.append(sum((gr.abs() * b).flatten(1).sum(1) for gr, b in zip(grads, bs)))
        return torch.cat(out)
    return feats.detach().contiguous(), bound


def feats_check_indices(err, shape, worst=32):
    """Where seanet_ref's bound is evaluated: the first and the last row of feats [Te][He] (the causal start, the clip's end) and
    the `worst` elements with the largest error.  err: the flat |error|."""
    Te, He = shape
    return torch.cat([torch.arange(He), torch.arange((Te - 1) * He, Te * He), err.topk(min(worst, err.numel())).indices]).unique()


def downsample_ref(W, tf):
    """The stride-2, k = 4 conv with replicate padding on the GPU's OWN transformer output tf [Te][He] (float32, exact input: only the
    planes' 16 bits and the float32 sums enter the bound) -> (emb [Tf][He] float64, bound)."""
    a = Bounded(torch.as_tensor(tf).to(F64).T[None])
    o = _conv_bounded(a, W["enc.downsample.weight"], None, stride=2, pad_mode="replicate")
    return o.v[0].T.contiguous(), o.err[0].T.contiguous()


def projection_ref(W, emb, which):
    """sem / aco = the 1x1 projection of the GPU's OWN emb [Tf][He] -> ([Tf][vq_dim] float64, bound), as downsample_ref."""
    w = W[f"enc.vq.{which}.input_proj.weight"]
    a = Bounded(torch.as_tensor(emb).to(F64).T[None])
    o = _conv_bounded(a, w[:, :, None], None)
    return o.v[0].T.contiguous(), o.err[0].T.contiguous()
