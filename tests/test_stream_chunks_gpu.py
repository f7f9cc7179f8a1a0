"""rt_stream_chunks (the chunks of several listeners in one launch) against rt_stream_chunk (one chunk per call): output bytes, length,
dc and gain identical per item - the two kernels share one body.  Five items per call with the flags a session meets (first, middle,
last, first-and-last, a silent first chunk that reports gain 0), at the lengths where the kernel changes path."""
import pytest
import torch

from rho_tts_amd import _native

pytestmark = pytest.mark.gpu

SR = 24000


@pytest.fixture(scope="module")
def ctx():
    c = _native.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def len12(ctx):
    """wav_length(12): the first piece of a streamed segment at the default chunk size (preset small)"""
    from rho_tts_amd import config
    from rho_tts_amd._native_model import NativeModel
    nm = NativeModel(ctx, config.small(), max_batch=2)
    try:
        n = nm.wav_length(12)
    finally:
        nm.close()
    assert 2 * 480 < n <= 12 * config.small().codec.total_upsample       # (n frames decode to n * up - d samples)
    return n


def speech(n, seed, silent=False):
    """n samples: a quiet lead-in, a modulated tone, a quiet tail (so trims, the audible span and the fades all have work)"""
    g = torch.Generator().manual_seed(seed)
    if silent or n == 0:
        return torch.zeros(n)
    t = torch.arange(n, dtype=torch.float32) / SR
    x = 0.2 * torch.sin(2 * torch.pi * 180.0 * t) * (0.5 + 0.5 * torch.sin(2 * torch.pi * 7.0 * t)) + 0.02 * torch.randn(n, generator=g)
    lead, tail = n // 5, n // 7
    x[:lead] *= 1e-4
    x[n - tail:] *= 1e-4
    return x + 0.003


KINDS = [("first", True, False, False), ("middle", False, False, False), ("last", False, True, False), ("whole", True, True, False),
         ("silent first", True, False, True)]


def alone_and_together(ctx, p, lengths, order):
    """five items (KINDS) with `lengths`, given to rt_stream_chunks in `order`; every one against its own rt_stream_chunk call"""
    xs, states, flags = [], [], []
    for k, ((name, first, last, silent), n) in enumerate(zip(KINDS, lengths)):
        xs.append(speech(n, 100 + k, silent).cuda())
        states.append([0.0, 0.0] if first else [0.0125, 1.75])         # a carried (dc, gain) for the chunks that do not measure
        flags.append(_native.Context.stream_flags(first, last))
    want = []
    for x, st, (name, first, last, _) in zip(xs, states, KINDS):
        s = list(st)
        y = ctx.stream_chunk(p, x, s, first, last)
        want.append((y.cpu().clone(), s))
    st_in = [list(states[i]) for i in order]
    got = ctx.stream_chunks(p, [xs[i] for i in order], st_in, [flags[i] for i in order])
    for j, i in enumerate(order):
        y, s = want[i]
        assert got[j].numel() == y.numel(), (KINDS[i][0], lengths[i], got[j].numel(), y.numel())
        assert torch.equal(got[j].cpu().view(torch.int32), y.view(torch.int32)), (KINDS[i][0], lengths[i])
        if lengths[i] == 0:
            assert st_in[j] == states[i] and got[j].numel() == 0       # nothing written, the state kept
        else:
            assert st_in[j] == s, (KINDS[i][0], lengths[i], st_in[j], s)
    return want


def test_every_item_is_what_rt_stream_chunk_gives_it_alone(ctx, len12):
    p = _native.make_post_params(sample_rate=SR, stages=0)
    W, F = p.window, p.fade
    assert W == 240 and F == 480
    for n in (0, 1, W - 1, 2 * F - 1, 2 * F, 4567, len12):
        want = alone_and_together(ctx, p, [n] * 5, [0, 1, 2, 3, 4])
        if n >= W:
            assert want[4][1][1] == 0.0 and want[0][1][1] > 0.0          # the silent first chunk reports gain 0, the audible one a gain
    # mixed lengths in one call, and the same items in another order
    mixed = [len12, 4567, 2 * F - 1, 2 * F, W - 1]
    alone_and_together(ctx, p, mixed, [0, 1, 2, 3, 4])
    alone_and_together(ctx, p, mixed, [4, 2, 0, 3, 1])
    alone_and_together(ctx, p, [0, len12, 0, 1, 4567], [3, 0, 4, 1, 2])


def test_bad_arguments_are_refused(ctx):
    p = _native.make_post_params(sample_rate=SR, stages=0)
    x = torch.zeros(8, device="cuda")
    assert ctx.stream_chunks(p, [], [], []) == []
    bad = _native.make_post_params(sample_rate=SR, stages=0)
    bad.window = 1
    with pytest.raises(ValueError):
        ctx.stream_chunks(bad, [x], [[0.0, 0.0]], [0])
