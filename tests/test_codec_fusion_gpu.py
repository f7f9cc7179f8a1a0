"""The codec decoder's fused 192-channel residual units (k_conv_win<4, 1, 1, 6, FUSE>: k = 7 conv, SnakeBeta, 1x1 conv, residual
and the next unit's planes in one launch, weight fragments staged through LDS), the dropped residual-stream store of every
stage's third unit and the last conv writing the caller's buffer.  Each is a rt_debug_tune pair (3000 / 3001, 2900 / 2901) and
none may change a bit of the waveform: the fused unit multiplies the same hi / lo planes in the same K order (chunk, tap, hi
before lo; the 1x1 conv's k-tiles ascending) and runs the same epilogue arithmetic as the two launches it replaces.

The `small` preset has a 384-channel decoder with rates 4 / 3 / 2: a 192-, a 96- and a 48-channel stage.  The 0.6B preset carries the
real codec (1536 channels, rates 8 / 5 / 4 / 3: 768 / 384 / 192 / 96).  Every item starts with taps that reach before its first
row (causal zero padding), and the row counts below are not multiples of the 128-row tile, so items begin inside tiles and the
last tile is partial.
"""
import ctypes as C

import pytest
import torch

from rho_tts_amd import config, weights

pytestmark = pytest.mark.gpu

NEW_KNOBS = ((2900, 2901), (3000, 3001))          # (off, on) per change of this file's subject


@pytest.fixture(scope="module")
def ctx():
    from rho_tts_amd import _native
    c = _native.Context(0)
    yield c
    c.close()


def load(ctx, preset, max_batch, **kw):
    from rho_tts_amd._native_model import NativeModel
    cfg = config.PRESETS[preset]()
    state = weights.synthetic_state(cfg, 789, device="cuda")
    nm = NativeModel(ctx, cfg, max_batch=max_batch, **kw)
    nm.load_state(state)
    del state
    torch.cuda.empty_cache()
    return cfg, nm


@pytest.fixture(scope="module")
def small(ctx):
    cfg, nm = load(ctx, "small", 8, max_codec_frames=40)
    yield cfg, nm
    nm.close()


def rand_codes(cfg, lens, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, cfg.codec.codebook_size, (n, cfg.codec.num_quantizers), generator=g) for n in lens]


def with_knobs(nm, codes_off, fn):
    """fn() with the given rt_debug_tune codes applied; the defaults (the `on` codes) are restored afterwards."""
    try:
        for code in codes_off:
            assert nm.lib.rt_debug_tune(code, 0) == 0
        return fn()
    finally:
        for _, on in NEW_KNOBS:
            nm.lib.rt_debug_tune(on, 0)


def assert_same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.shape == y.shape and torch.equal(x, y)
        assert float(x.abs().max()) > 0.01               # not a comparison of silence


@pytest.mark.parametrize("off", [(3000,), (2900,), (2900, 3000)])
def test_each_new_form_equals_the_unfused_route_small(small, off):
    cfg, nm = small
    codes = rand_codes(cfg, [7, 12, 9, 1, 33], 9)        # 33 frames: 524 rows at 192 channels per item, 2620 in the batch
    new = [w.clone() for w in nm.code2wav(codes)]
    old = with_knobs(nm, off, lambda: [w.clone() for w in nm.code2wav(codes)])
    assert_same(new, old)


def test_tap_unrolling_off_takes_the_two_launch_route_small(small):
    """The fused 192-channel unit exists as the tap-unrolled kernel only: with rt_debug_tune 2600 the pairs run as two launches
    whatever 3000 / 3001 says, and the bits stay."""
    cfg, nm = small
    codes = rand_codes(cfg, [12, 5], 4)
    try:
        assert nm.lib.rt_debug_tune(2600, 0) == 0
        new = [w.clone() for w in nm.code2wav(codes)]
        old = with_knobs(nm, (3000,), lambda: [w.clone() for w in nm.code2wav(codes)])
    finally:
        nm.lib.rt_debug_tune(2601, 0)
    assert_same(new, old)
    assert_same(new, [w.clone() for w in nm.code2wav(codes)])


def test_item_alone_equals_item_beside_a_longer_one_small(small):
    cfg, nm = small
    codes = rand_codes(cfg, [7, 33, 12], 11)
    wavs = [w.clone() for w in nm.code2wav(codes)]
    for c, w in zip(codes, wavs):
        assert torch.equal(nm.code2wav([c])[0], w)
    assert_same(wavs[:1], [nm.code2wav(codes[:2])[0].clone()])


def test_last_conv_writes_a_strided_caller_buffer(small):
    """wav_stride wider than the waveform: every item's samples land in its own row and the padding behind them is not touched."""
    cfg, nm = small
    codes = rand_codes(cfg, [9, 12], 5)
    ref = [w.clone() for w in nm.code2wav(codes)]
    B, T, Q = len(codes), 12, cfg.codec.num_quantizers
    L = nm.wav_length(T)
    buf = torch.zeros(B, T, Q, dtype=torch.int32)
    for b, c in enumerate(codes):
        buf[b, : c.shape[0]] = c.to(torch.int32)
    for off in ((), (2900,)):
        wav = torch.full((B, L + 37), 7.0, dtype=torch.float32, device="cuda")
        nfr, lens = (C.c_int32 * B)(9, 12), (C.c_int64 * B)()
        torch.cuda.synchronize()

        def run():
            nm.ctx.check(nm.lib.rt_code2wav(nm.handle, B, T, C.cast(buf.data_ptr(), C.POINTER(C.c_int32)), nfr, C.c_void_p(wav.data_ptr()), L + 37, lens),
                         "rt_code2wav")
        with_knobs(nm, off, run)
        for b in range(B):
            assert torch.equal(wav[b, : lens[b]], ref[b])
        assert bool((wav[:, L:] == 7.0).all())


def test_real_codec_dimensions_new_defaults_equal_all_new_knobs_off(ctx):
    """The real codec decoder, 32 items of 44 frames as in bench.py (84 480 rows per item at 96 channels): the 256-row fused 96-channel
    units, the fused 192-channel units and the unfused 384- / 768-channel units all lose their third unit's residual-stream store."""
    cfg, nm = load(ctx, "0.6b", 32, max_positions=256)
    try:
        codes = rand_codes(cfg, [44] * 31 + [29], 3)
        new = [w.clone() for w in nm.code2wav(codes)]
        old = with_knobs(nm, (2900, 3000), lambda: [w.clone() for w in nm.code2wav(codes)])
        assert_same(new, old)
        only192 = with_knobs(nm, (3000,), lambda: [w.clone() for w in nm.code2wav(codes)])
        assert_same(new, only192)
        # one item alone against the same item in the batch
        assert torch.equal(nm.code2wav([codes[-1]])[0], new[-1])
        assert torch.equal(nm.code2wav([codes[0]])[0], new[0])
    finally:
        nm.close()
