"""Long contexts and sliding windows at the real model dimensions: the sizes a user reaches with ordinary inputs (a 60-s
reference clip, a 15-s segment), which the rest of the suite stops short of.

Kernel level (a-c): the decode attention at up to 4096 positions behind voice prefixes of 1024 / 2047 / 2048 rows on all three
routes, the prompt prefill behind prefixes of 1023..2000 rows and the prefix's own prefill at 1024..2048 rows, and the sliding-
window attention at the codec (16 / 16 x 64, W = 72) and encoder (8 / 8 x 64, W = 250) geometries on both cache forms (bf16, and
hi + lo bf16 planes with a float32 output).  Which keys a row reads is pinned EXACTLY by the key census (q = 0 makes the softmax
uniform, V[p] = indicator of p mod d, so every output is a count of visible keys over their number).  Random data is compared to
float64 with an element-wise bound, and every such bound is backed by a sensitivity control: the test's own reference, recomputed
with the window or the prefix length moved by one key, must differ from the true one by at least 10x the bound somewhere in every
affected row - a bound that could not see one key would be a test bug.  The reused decode-attention helper's float32 comparison
(tolerance 1e-2 of the output scale) cannot see one key in 4096 and is kept as an arithmetic check only: there the census carries
key selection.

Model level (e-g): the codec decoder past its 72-frame window and through Engine.vocode's chunking, the audio encoder past its
250-position window (a 30-s clip), and teacher-forced logits of the 0.6B preset behind a 2085-row voice prefix at the default
4096 positions - the only check that reaches the production layout of the tiled prefix buffers (sized from max_positions).
"""
import time

import pytest
import torch

from tests.test_encoder_gpu import check_codes, clip
from tests.test_gemm_col_gpu import _fused_attention_key_census, _fused_attention_matches_fp32
from tests.test_kernels_gpu import _prefill_attention
from tests.test_model_shapes_gpu import MAX_CAP, MAX_SLACK, RMS_CAP, RMS_SLACK, clone_voice, sentences

pytestmark = pytest.mark.gpu

BF16_REL = 2.0 ** -8          # round-to-nearest bf16: |bf16(x) - x| <= 2^-8 |x|


@pytest.fixture(scope="module")
def ctx():
    from rho_tts_amd import _native
    c = _native.Context(0)
    yield c
    c.close()


@pytest.fixture(autouse=True)
def wall_time(request):
    """Per-test wall time (CPU oracle work included), printed with the test's output."""
    n = torch.get_num_threads()
    torch.set_num_threads(min(n, 16))
    t0 = time.perf_counter()
    yield
    torch.set_num_threads(n)
    print(f"\n[wall] {request.node.name}: {time.perf_counter() - t0:.1f} s")


# ---------------------------------------------------------------------------------------------------------------- references
def attention_ref(q, k, v, slot, lo, hi, prefix_slot=-1, Lp=0):
    """float64 softmax(q k^T / sqrt(d)) v of rows q [M][heads][d] over cache positions [lo[r], hi[r]] of slot[r]; positions
    below Lp are read from prefix_slot.  k / v [slots][kv_heads][max_pos][d] (any float type).  Returns [M][heads * d]."""
    M, heads, d = q.shape
    kvh, P = k.shape[1], k.shape[2]
    rep = heads // kvh
    out = torch.empty(M, heads, d, dtype=torch.float64)
    p = torch.arange(P)
    for s in slot.unique().tolist():
        rows = (slot == s).nonzero().flatten()
        K, V = k[s].double(), v[s].double()
        if Lp > 0:
            K = torch.cat([k[prefix_slot, :, :Lp].double(), K[:, Lp:]], 1)
            V = torch.cat([v[prefix_slot, :, :Lp].double(), V[:, Lp:]], 1)
        K, V = K.repeat_interleave(rep, 0), V.repeat_interleave(rep, 0)
        for c0 in range(0, rows.numel(), 128):
            r = rows[c0:c0 + 128]
            sc = torch.einsum("mhd,hpd->mhp", q[r].double(), K) * d ** -0.5
            mask = (p[None] < lo[r, None]) | (p[None] > hi[r, None])
            sc.masked_fill_(mask[:, None], float("-inf"))
            out[r] = torch.einsum("mhp,hpd->mhd", torch.softmax(sc, -1), V)
    return out.reshape(M, heads * d)


def bf16_bound(ref, eps):
    """element-wise bound for a bf16 output of a float32 computation: its rounding plus eps of accumulated float32 error"""
    return BF16_REL * ref.abs() + eps


def check_with_sensitivity(got, ref, tol, perturbed, affected, what):
    """|got - ref| <= tol element-wise; and for every perturbed reference (one key more or less), every affected row moves by
    >= 10 x tol somewhere - the bound can see one key in each of those rows."""
    err = ((got.double() - ref).abs() / tol).max(1).values
    assert float(err.max()) <= 1.0, (what, float(err.max()), int(err.argmax()))
    for name, alt in perturbed:
        see = ((alt - ref).abs() / tol).max(1).values[affected]
        assert float(see.min()) >= 10.0, (what, name, float(see.min()))
    return float(err.max())


def census_v(slots, kvh, max_pos, d):
    ind = torch.zeros(max_pos, d)
    ind[torch.arange(max_pos), torch.arange(max_pos) % d] = 1.0
    return ind[None, None].expand(slots, kvh, max_pos, d).contiguous()


def census_want(lo, hi, d):
    """[M][d]: the share of the visible positions [lo, hi] congruent to each j mod d (float32, as the kernel divides)"""
    rows = []
    for a, b in zip(lo.tolist(), hi.tolist()):
        cnt = torch.bincount(torch.arange(a, b + 1) % d, minlength=d).float()
        rows.append(cnt / float(b - a + 1))
    return torch.stack(rows)


# ---------------------------------------------------------------------------------------------------------------- a. decode
DECODE_CASES = [(1024, 0), (1024, 1), (1024, 2), (2047, 0), (2047, 1), (2047, 2), (2048, 0), (2048, 1), (2048, 2), (0, 0)]


@pytest.mark.parametrize("Lp,route", DECODE_CASES, ids=[f"Lp{a}-route{b}" for a, b in DECODE_CASES])
def test_fused_decode_attention_at_4096_positions(ctx, Lp, route):
    """rt_debug_attention_fused at max_pos 4096 (1.7B / 0.6B talker heads 16 / 8 x 128, 32 rows), positions up to 4095, behind a
    prefix of 1024 / 2047 / 2048 rows or none; route 0 = vector unit, 1 / 2 = matrix cores with four rows / one row per
    workgroup (rt_debug_tune 1500 + route).  The exact key census and the float32 comparison of tests/test_gemm_col_gpu.py."""
    ctx.lib.rt_debug_tune(1500 + route, 0)
    try:
        _fused_attention_key_census(ctx, 128, 16, 8, 4096, 32, Lp, Lp, 4095)
        _fused_attention_matches_fp32(ctx, 128, 16, 8, 4096, 32, Lp, Lp, 4095)
    finally:
        ctx.lib.rt_debug_tune(1500, 0)


# ---------------------------------------------------------------------------------------------------------------- b. prefill
@pytest.mark.parametrize("Lp,M", [(1023, 300), (1024, 1100), (2000, 700)])
def test_prefill_attention_behind_long_prefixes(ctx, Lp, M):
    """Prompt rows behind a shared prefix of 1023 / 1024 / 2000 rows (1.7B heads), up to 1100 rows in one launch, on the vector
    unit (mode 0) and the matrix cores (mode 1): exact census on both; mode 0 against float64 with the bf16 bound backed by the
    prefix-length +-1 sensitivity control; mode 1 (bf16 MFMA operands) against float64 at the existing test's 2e-2, against
    mode 0, and batch invariance bit for bit."""
    d, heads, kvh, slots = 128, 16, 8, 5
    max_pos = Lp + 96
    g = torch.Generator().manual_seed(500 + Lp)
    k = torch.randn(slots, kvh, max_pos, d, generator=g).to(torch.bfloat16)
    v = torch.randn(slots, kvh, max_pos, d, generator=g).to(torch.bfloat16)
    q = torch.randn(M, heads, d, generator=g)
    prefix_slot = slots - 1
    slot = torch.randint(0, slots - 1, (M,), generator=g).to(torch.int32)
    pos = (Lp + torch.randint(0, 96, (M,), generator=g)).to(torch.int32)
    pos[0], pos[1] = Lp, max_pos - 1
    kd, vd, qd, slot_d, pos_d = k.cuda(), v.cuda(), q.cuda(), slot.cuda(), pos.cuda()
    lo = torch.zeros(M, dtype=torch.long)
    hi = pos.long()
    ref = attention_ref(q, k, v, slot.long(), lo, hi, prefix_slot, Lp)
    vec = _prefill_attention(ctx, qd, slot_d, pos_d, kd, vd, prefix_slot, Lp, 0).float().cpu()
    mfma = _prefill_attention(ctx, qd, slot_d, pos_d, kd, vd, prefix_slot, Lp, 1).float().cpu()
    eps = 2e-6 * float(v.float().abs().max())
    tol = bf16_bound(ref, eps)
    perturbed = [(f"prefix {Lp + e}", attention_ref(q, k, v, slot.long(), lo, hi, prefix_slot, Lp + e)) for e in (-1, 1)]
    worst = check_with_sensitivity(vec, ref, tol, perturbed, slice(None), f"mode 0 Lp {Lp}")
    e1 = float(((mfma.double() - ref).abs().max(1).values / ref.abs().max(1).values.clamp(min=1.0)).max())
    print(f"\nLp {Lp}, {M} rows: mode 0 worst err / bound {worst:.3f}; mode 1 max err {e1:.2e} of max(1, |ref|)")
    assert e1 < 2e-2, e1
    assert float((mfma - vec).abs().max()) < 3e-2
    for r in (0, 1, M // 2, M - 1):
        alone = _prefill_attention(ctx, qd[r:r + 1].contiguous(), slot_d[r:r + 1].contiguous(), pos_d[r:r + 1].contiguous(), kd, vd, prefix_slot, Lp, 1)
        assert torch.equal(alone[0].float().cpu(), mfma[r]), r
    perm = torch.randperm(M, generator=g)
    pc = perm.cuda()
    shuffled = _prefill_attention(ctx, qd[pc].contiguous(), slot_d[pc].contiguous(), pos_d[pc].contiguous(), kd, vd, prefix_slot, Lp, 1)
    assert torch.equal(shuffled.float().cpu(), mfma[perm])
    # key census: the prefix's rows from the prefix slot only, the own rows from the row's slot only (the other copies poisoned)
    v1 = census_v(slots, kvh, max_pos, d)
    v1[prefix_slot, :, Lp:] = 64.0
    v1[: slots - 1, :, :Lp] = 64.0
    v1 = v1.to(torch.bfloat16).cuda()
    want = census_want(lo, hi, d).to(torch.bfloat16).float()
    q0 = torch.zeros_like(qd)
    for mode in (0, 1):
        cen = _prefill_attention(ctx, q0, slot_d, pos_d, kd, v1, prefix_slot, Lp, mode).float().cpu().view(M, heads, d)
        if mode == 0:
            assert torch.equal(cen, want[:, None].expand(M, heads, d)), mode
        else:      # (P rounded to bf16 on the matrix cores: within one bf16 step of the count; a missing or extra key moves it >= 1/n)
            assert float((cen - want[:, None]).abs().max()) <= 2 ** -9 * float(want.max()), mode


@pytest.mark.parametrize("M", [1024, 1025, 2048])
def test_prefix_self_prefill_at_long_prefixes(ctx, M):
    """rt_debug_attention_prefill mode 2 (the voice prefix attending to itself, causal) at 1024 / 1025 / 2048 rows: exact census
    and float64 within the matrix-core bound of the existing test (2e-2 of the output scale)."""
    d, heads, kvh, slots, max_pos = 128, 16, 8, 2, M + 32
    g = torch.Generator().manual_seed(700 + M)
    k = torch.randn(slots, kvh, max_pos, d, generator=g).to(torch.bfloat16)
    v = torch.randn(slots, kvh, max_pos, d, generator=g).to(torch.bfloat16)
    q = torch.randn(M, heads, d, generator=g)
    slot = torch.ones(M, dtype=torch.int32)
    pos = torch.arange(M, dtype=torch.int32)
    kd, vd, qd, slot_d, pos_d = k.cuda(), v.cuda(), q.cuda(), slot.cuda(), pos.cuda()
    out = _prefill_attention(ctx, qd, slot_d, pos_d, kd, vd, 1, M, 2).float().cpu()
    rows = torch.tensor(sorted(set(list(range(0, M, 61)) + [7, 8, 31, 32, 1023, M - 2, M - 1])))
    ref = attention_ref(q[rows], k, v, slot[rows].long(), torch.zeros(rows.numel(), dtype=torch.long), pos[rows].long())
    e = float(((out[rows].double() - ref).abs().max(1).values / ref.abs().max(1).values.clamp(min=1.0)).max())
    assert e < 2e-2, e
    v1 = census_v(slots, kvh, max_pos, d).to(torch.bfloat16).cuda()
    cen = _prefill_attention(ctx, torch.zeros_like(qd), slot_d, pos_d, kd, v1, 1, M, 2).float().cpu().view(M, heads, d)
    want = census_want(torch.zeros(M, dtype=torch.long), pos.long(), d).to(torch.bfloat16).float()
    assert float((cen - want[:, None]).abs().max(2).values.max(1).values.div(want.max(1).values).max()) <= 2 ** -9


# ---------------------------------------------------------------------------------------------------------------- c. windows
def _windowed(ctx, planes, q, k, v, slot, pos, window):
    """rt_debug_attention (bf16 caches, bf16 out) or rt_debug_attention_planes (hi + lo planes, float32 out) on float32 K / V"""
    M, heads, d = q.shape
    slots, kvh, max_pos = k.shape[0], k.shape[1], k.shape[2]
    qd, sd, pd = q.cuda(), slot.to(torch.int32).cuda(), pos.to(torch.int32).cuda()
    if planes:
        khi, vhi = k.to(torch.bfloat16), v.to(torch.bfloat16)
        klo, vlo = (k - khi.float()).to(torch.bfloat16), (v - vhi.float()).to(torch.bfloat16)
        bufs = [t.cuda() for t in (khi, klo, vhi, vlo)]
        out = torch.full((M, heads * d), float("nan"), device="cuda")
        torch.cuda.synchronize()
        ctx.check(ctx.lib.rt_debug_attention_planes(ctx.handle, qd.data_ptr(), M, heads, kvh, d, sd.data_ptr(), pd.data_ptr(), window,
                                                    *[b.data_ptr() for b in bufs], slots, max_pos, out.data_ptr()), "rt_debug_attention_planes")
    else:
        kd, vd = k.to(torch.bfloat16).cuda(), v.to(torch.bfloat16).cuda()
        out = torch.full((M, heads * d), float("nan"), dtype=torch.bfloat16, device="cuda")
        torch.cuda.synchronize()
        ctx.check(ctx.lib.rt_debug_attention(ctx.handle, qd.data_ptr(), M, heads, kvh, d, sd.data_ptr(), pd.data_ptr(), window,
                                             kd.data_ptr(), vd.data_ptr(), slots, max_pos, out.data_ptr()), "rt_debug_attention")
    torch.cuda.synchronize()
    return out.float().cpu()


def _window_rows(geometry):
    """(heads, kv_heads, d, window, slots, max_pos, slot [M], pos [M]) of the launch"""
    if geometry.startswith("codec"):      # rt_code2wav: B items x T frames in one launch, row (b, t) at slot b, position t
        B, T = 4, 325
        slot = torch.arange(B).repeat_interleave(T)
        pos = torch.arange(T).repeat(B)
        return 16, 16, 64, 72 if geometry == "codec" else 0, B, T, slot, pos
    n = int(geometry.split("-")[1])       # encoder transformer: one item, 2 x frames positions
    W = 0 if geometry.endswith("w0") else 250
    if n <= 750:
        return 8, 8, 64, W, 1, n, torch.zeros(n, dtype=torch.long), torch.arange(n)
    g = torch.Generator().manual_seed(n)
    edge = torch.tensor([0, 1, 248, 249, 250, 251, 252, 499, 500, 501, 2047, 2048, n - 2, n - 1])
    pos = torch.cat([edge, torch.randint(0, n, (178,), generator=g)])
    return 8, 8, 64, W, 2, n, torch.arange(pos.numel()) % 2, pos


WINDOW_CASES = ["codec", "codec-w0", "enc-750", "enc-4096", "enc-750-w0", "enc-4096-w0"]


@pytest.mark.parametrize("planes", [False, True], ids=["bf16", "planes"])
@pytest.mark.parametrize("geometry", WINDOW_CASES)
def test_sliding_window_attention_at_real_geometry(ctx, geometry, planes):
    """The codec pre-transformer (16 / 16 x 64, W = 72, 4 items x 325 frames in one launch) and the encoder transformer (8 / 8 x
    64, W = 250, 750 and 4096 positions), and W = 0, on the bf16 cache (bf16 out) and the hi + lo plane cache (float32 out, the
    form both stacks run).  Positions W-2 .. W+1 and max_pos-1 included.  Exact census; random data against float64 with the
    window +-1 sensitivity control (W = 0: the first key dropped)."""
    heads, kvh, d, W, slots, max_pos, slot, pos = _window_rows(geometry)
    M = pos.numel()
    assert max_pos - 1 in pos.tolist() and (W == 0 or {W - 2, W - 1, W, W + 1} <= set(pos.tolist()))
    hi = pos.long()
    lo = (hi - W + 1).clamp(min=0) if W else torch.zeros(M, dtype=torch.long)
    g = torch.Generator().manual_seed(1000 + M + W)
    k = torch.randn(slots, kvh, max_pos, d, generator=g)
    v = torch.randn(slots, kvh, max_pos, d, generator=g)
    q = torch.randn(M, heads, d, generator=g)
    kq, vq = (k, v) if planes else (k.to(torch.bfloat16).float(), v.to(torch.bfloat16).float())   # the bf16 cache holds bf16(K / V)
    # census: q = 0, V = indicator of p mod d (exact in bf16 and as hi + lo)
    want = census_want(lo, hi, d)
    cen = _windowed(ctx, planes, torch.zeros(M, heads, d), k, census_v(slots, kvh, max_pos, d), slot, pos, W).view(M, heads, d)
    want = want if planes else want.to(torch.bfloat16).float()
    assert torch.equal(cen, want[:, None].expand(M, heads, d)), float((cen - want[:, None]).abs().max())
    # random data against float64
    got = _windowed(ctx, planes, q, k, v, slot, pos, W)
    ref = attention_ref(q, kq, vq, slot, lo, hi)
    vmax = float(v.abs().max())
    # planes: value = hi + lo (<= 2^-17 relative from float32), float32 accumulation and output - about 1e-5 of the values' scale;
    # bf16: the output's own rounding plus the same float32 error
    tol = torch.full_like(ref, 5e-6 * vmax) if planes else bf16_bound(ref, 2e-6 * vmax)
    if W:
        perturbed = [(f"window {W + e}", attention_ref(q, kq, vq, slot, (hi - (W + e) + 1).clamp(min=0), hi)) for e in (-1, 1)]
        affected = hi >= W
    else:
        perturbed = [("first key dropped", attention_ref(q, kq, vq, slot, torch.ones(M, dtype=torch.long), hi))]
        affected = hi >= 1
    worst = check_with_sensitivity(got, ref, tol, perturbed, affected, f"{geometry} planes={planes}")
    print(f"\n{geometry} ({'planes' if planes else 'bf16'}): {M} rows, W {W}, worst err / bound {worst:.3f}")


# ---------------------------------------------------------------------------------------------------------------- e. codec decoder
def test_code2wav_past_the_window_and_chunked_vocode(ctx):
    """The codec decoder of the 0.6B preset past its 72-frame window: items of 73, 160 and 325 frames (max_codec_frames) and a
    37-frame one in ONE rt_code2wav call, RMSE < 1e-3 against the float32 oracle, each alone bit-equal to itself in the batch;
    Engine.vocode on 340 and 601 frames (chunks of 300 + 25 frames of context) against the oracle's chunked_code2wav."""
    from oracle.model import OracleModel
    from rho_tts_amd import config, weights
    from rho_tts_amd.engine import Engine
    cfg = config.PRESETS["0.6b"]()
    eng = Engine(cfg=cfg, model_path="0.6b", device_ordinal=0, max_batch=4, weight_seed=789, synthetic=True, max_positions=256)
    try:
        nm = eng.model
        assert nm.max_codec_frames == 325
        om = OracleModel(cfg, weights.synthetic_state(cfg, 789, only_prefix="codec."))
        g = torch.Generator().manual_seed(19)
        Q = cfg.codec.num_quantizers
        codes = [torch.randint(0, cfg.codec.codebook_size, (n, Q), generator=g) for n in (73, 160, 325, 37)]
        wavs = nm.code2wav(codes)
        for c, w in zip(codes, wavs):
            with torch.no_grad():
                ref = om.code2wav(c.T[None])[0]
            assert w.shape[0] == ref.shape[0] == nm.wav_length(c.shape[0])
            rmse = float(torch.sqrt(torch.mean((w.cpu() - ref) ** 2)))
            print(f"\ncode2wav {c.shape[0]} frames in a batch of 4: rmse {rmse:.2e}")
            assert rmse < 1e-3, (c.shape[0], rmse)
            assert float(ref.abs().max()) > 0.05
            assert torch.equal(nm.code2wav([c])[0], w), c.shape[0]
        long = [torch.randint(0, cfg.codec.codebook_size, (n, Q), generator=g) for n in (340, 601)]
        for c, w in zip(long, eng.vocode([x.cuda() for x in long])):
            with torch.no_grad():
                ref = om.chunked_code2wav(c.T[None])[0]
            assert w.shape[0] == ref.shape[0]
            rmse = float(torch.sqrt(torch.mean((w.cpu() - ref) ** 2)))
            print(f"vocode {c.shape[0]} frames (chunked): rmse {rmse:.2e}")
            assert rmse < 1e-3, (c.shape[0], rmse)
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------------------------- f. encoder
def test_audio_encoder_past_its_window(ctx):
    """A 30-s clip (375 frames = 750 transformer positions against the 250-position window) through the encoder of the 0.6B preset
    at the default 4096 positions: codes exact or near-ties under check_codes' 1e-4 rule (at most 3), speaker embedding within
    1e-4; and the causal prefix property at the window's edge - frame 125 is transformer position 250."""
    from oracle import encoder as E
    from rho_tts_amd import config, weights
    from rho_tts_amd._native_model import NativeModel
    cfg = config.PRESETS["0.6b"]()
    state = weights.synthetic_state(cfg, 789, device="cuda")
    nm = NativeModel(ctx, cfg, max_batch=2)
    try:
        nm.load_state(state)
        W = {k: v.float().cpu() for k, v in state.items() if k.startswith("enc.")}
        del state
        torch.cuda.empty_cache()
        pcm = clip(cfg, 375, 5)
        codes, spk = nm.encode_voice(pcm)
        want, spk_o, mid = E.encode(W, cfg, pcm, return_intermediates=True)
        assert codes.shape == want.shape == (375, cfg.codec.num_quantizers)
        flips = check_codes(cfg, W, pcm, codes, want, mid)
        print(f"\n30-s clip: {flips} near-tie frames")
        assert flips <= 3
        assert float((spk - spk_o).abs().max()) < 1e-4 * max(1.0, float(spk_o.abs().max()))
        for n in (124, 125, 126):
            c, _ = nm.encode_voice(pcm, max_frames=n)
            assert torch.equal(c, codes[:n]), n
    finally:
        nm.close()


# ---------------------------------------------------------------------------------------------------------------- g. long prefix
def test_teacher_forced_logits_behind_a_2085_row_prefix(ctx):
    """0.6B, batch 4, the default 4096 positions (the tiled prefix buffers in their production layout), a 160-s voice prompt:
    2000 reference frames -> a 2085-row shared prefix; 3 frames teacher-forced on the oracle's greedy trajectory, decode positions
    past 2085.  Same self-calibrated bound as test_teacher_forced_logits_at_bench_shapes."""
    from oracle.model import OracleModel, Voice
    from oracle.sampling import SamplingParams
    from rho_tts_amd import config, weights
    from rho_tts_amd._native_model import NativeModel, RtSampling
    from rho_tts_amd.tokenizer import HashTokenizer
    cfg = config.PRESETS["0.6b"]()
    B, n_frames = 4, 3
    tok = HashTokenizer(cfg.text_vocab)
    state = weights.synthetic_state(cfg, 789, device="cuda")
    nm = NativeModel(ctx, cfg, max_batch=B)
    try:
        assert nm.max_positions == 4096
        nm.load_state(state)
        cpu_state = {k: v.cpu() for k, v in state.items()}
        om, om32 = OracleModel(cfg, cpu_state, act_bf16=True), OracleModel(cfg, cpu_state)
        del state
        torch.cuda.empty_cache()
        cond = clone_voice(cfg, tok, seconds=160.0)
        v = Voice(cond.language, None, cond.speaker_embed, cond.ref_text_ids, cond.ref_codes)
        n_prefix = nm.set_voice(v.language, None, v.speaker_embed, v.ref_text_ids, v.ref_codes)
        assert n_prefix == 2085, n_prefix                             # 3 role + 4 control + speaker + bos + 75 words + codec_bos + 2000 frames
        texts = [tok.encode(t) for t in sentences(B, 10, 791)]
        frames = [n_frames] * B
        tr_o, tr_32 = {}, {}
        with torch.no_grad():
            free = om.generate(v, texts, frames, SamplingParams(), trace=tr_o, share_prefix=True)
            om32.generate(v, texts, frames, SamplingParams(), trace=tr_32, share_prefix=True, forced_codes=free)
        codes, tr = nm.generate(texts, frames, RtSampling(0, 1.0, 1, 1.0, 1.0), forced_codes=free, trace=True)
        assert all(torch.equal(a, b) for a, b in zip(codes, free))
        V0, G1 = cfg.codec.codebook_size, cfg.n_groups - 1

        def dist(x, y, sig):
            e = (x - y).abs()
            return float(e.pow(2).mean().sqrt()) / sig, float(e.max()) / sig

        for name, o16, o32, gpu in (
                ("talker", torch.stack(tr_o["talker_logits"])[..., :V0], torch.stack(tr_32["talker_logits"])[..., :V0],
                 tr["talker"][:n_frames].cpu()[..., :V0]),
                ("predictor", torch.stack(tr_o["pred_logits"]).view(n_frames, G1, B, -1), torch.stack(tr_32["pred_logits"]).view(n_frames, G1, B, -1),
                 tr["predictor"][:n_frames].cpu())):
            sig = float(o16.std())
            floor_rms, floor_max = dist(o16, o32, sig)
            rms, mx = dist(gpu, o16, sig)
            print(f"\n{cfg.name} B={B} prefix {n_prefix} {name}: GPU vs bf16 oracle rms {rms:.5f} max {mx:.5f} sigma; "
                  f"bf16 vs f32 oracle rms {floor_rms:.5f} max {floor_max:.5f}")
            assert rms <= RMS_SLACK * floor_rms and rms <= RMS_CAP, (name, rms, floor_rms)
            assert mx <= MAX_SLACK * floor_max and mx <= MAX_CAP, (name, mx, floor_max)
            assert abs(float((gpu - o16).mean())) / sig < 2e-4
    finally:
        nm.close()
