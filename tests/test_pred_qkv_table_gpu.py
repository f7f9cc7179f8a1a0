"""The predictor's layer-0 q/k/v table (rt_model::pred_qkv0, built by rt_model_finalize): in passes 2..G-1 the launch that embeds
the drawn code copies that code's q/k/v row from the table and the layer-0 qkv GEMM launch is skipped (rt_debug_tune 3101, default).
The table is filled by the decode path's own launches, so the route must not move a single bit: every comparison here is
torch.equal between the table route (3101) and the GEMM route (3100) of the SAME model - codes, and where a static batch allows it
the talker and predictor logit traces."""
import dataclasses

import pytest
import torch

from rho_tts_amd import config
from rho_tts_amd.config import TransformerDims
from tests.test_model_gpu import build, make_voice, set_voice

pytestmark = pytest.mark.gpu

SAMPLED = (1, 0.9, 50, 1.0, 1.05)
GREEDY = (0, 1.0, 1, 1.0, 1.0)


@pytest.fixture(scope="module")
def ctx():
    from rho_tts_amd import _native
    c = _native.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module", params=["tiny", "small"])
def model16(request, ctx):
    """16 decode rows of the preset with a voice set: tiny has qw = 128 floats (fewer 16-byte pieces than sampler threads),
    small is the parity preset (hidden 256, head_dim 128, G = 8, Vp = 256)."""
    cfg = config.PRESETS[request.param]()
    nm, _ = build(ctx, cfg, max_batch=16)
    set_voice(nm, make_voice(cfg, True))
    yield cfg, nm
    nm.close()


def ragged(cfg, n, seed=3):
    g = torch.Generator().manual_seed(seed)
    texts = [[int(v) for v in torch.randint(0, cfg.text_vocab - 64, (int(k),), generator=g)] for k in torch.randint(1, 9, (n,), generator=g)]
    frames = [int(v) for v in torch.randint(3, 9, (n,), generator=g)]
    return texts, frames


def both_routes(nm, run):
    """run() with the GEMM route (3100), then with the table route (3101, the default that is left behind)"""
    try:
        nm.lib.rt_debug_tune(3100, 0)
        off = run()
    finally:
        nm.lib.rt_debug_tune(3101, 0)
    return off, run()


def same(off, on):
    (codes_off, tr_off), (codes_on, tr_on) = off, on
    assert len(codes_off) == len(codes_on) and all(torch.equal(a, b) for a, b in zip(codes_off, codes_on))
    for key in ("talker", "predictor"):
        assert torch.equal(tr_off[key], tr_on[key]), key


def test_same_run_with_the_table_off(model16):
    from rho_tts_amd._native_model import RtSampling
    cfg, nm = model16
    texts, frames = ragged(cfg, 16)
    off, on = both_routes(nm, lambda: nm.generate(texts, frames, RtSampling(*SAMPLED), seed=77, trace=True))
    same(off, on)
    assert len({tuple(c.flatten().tolist()) for c in on[0]}) > 1                   # (the rows do decode different things)


@pytest.mark.parametrize("other", [800, 200])
def test_same_run_on_the_other_routes(model16, other):
    """the unfused producer (800: k_embed_rowsq gathers the row, not the sampler) and eager frames (200: no captured graphs)"""
    from rho_tts_amd._native_model import RtSampling
    cfg, nm = model16
    texts, frames = ragged(cfg, 16)
    base = nm.generate(texts, frames, RtSampling(*SAMPLED), seed=77, trace=True)
    try:
        nm.lib.rt_debug_tune(other, 0)
        off, on = both_routes(nm, lambda: nm.generate(texts, frames, RtSampling(*SAMPLED), seed=77, trace=True))
    finally:
        nm.lib.rt_debug_tune(1 + other, 0)
    same(off, on)
    same(base, on)


def test_forced_codes_take_the_forced_row(model16):
    """teacher forcing: the producer embeds the code it WRITES, and the gather must follow that code, not the arg-max"""
    from rho_tts_amd._native_model import RtSampling
    cfg, nm = model16
    texts, frames = ragged(cfg, 16)
    drawn = nm.generate(texts, frames, RtSampling(*SAMPLED), seed=77)
    off, on = both_routes(nm, lambda: nm.generate(texts, frames, RtSampling(*GREEDY), forced_codes=drawn, trace=True))
    same(off, on)
    assert all(torch.equal(a, b) for a, b in zip(on[0], drawn))
    free = nm.generate(texts, frames, RtSampling(*GREEDY))
    assert not all(torch.equal(a, b) for a, b in zip(free, drawn))                 # (forcing did change what is embedded)


def test_rows_that_join_mid_run(ctx):
    """more items than rows: queued items take over finished rows between two frames and go through the same producers"""
    from rho_tts_amd._native_model import RtSampling
    cfg = config.PRESETS["tiny"]()
    nm, _ = build(ctx, cfg, max_batch=4)
    try:
        set_voice(nm, make_voice(cfg, True))
        g = torch.Generator().manual_seed(17)
        n = 13
        texts = [[int(v) for v in torch.randint(0, cfg.text_vocab - 64, (int(k),), generator=g)] for k in torch.randint(1, 9, (n,), generator=g)]
        frames = [int(v) for v in torch.randint(3, 15, (n,), generator=g)]
        ids = [100 + 7 * i for i in range(n)]

        def run():
            out = nm.generate(texts, frames, RtSampling(*SAMPLED), seed=5, item_ids=ids)
            return out, nm.generate_stats()
        (off, st_off), (on, st_on) = both_routes(nm, run)
        assert st_on["rows"] == 4 and st_on["hand_overs"] >= 2 and st_on == st_off
        assert [c.shape[0] for c in on] == frames
        assert all(torch.equal(a, b) for a, b in zip(off, on))
    finally:
        nm.close()


def test_three_rows(ctx):
    """an odd batch on the tiny preset: 3 rows of a 32-row tile, a 128-float q/k/v row against 256 sampler threads"""
    from rho_tts_amd._native_model import RtSampling
    cfg = config.PRESETS["tiny"]()
    nm, _ = build(ctx, cfg, max_batch=3)
    try:
        set_voice(nm, make_voice(cfg, True))
        texts, frames = ragged(cfg, 3, seed=11)
        same(*both_routes(nm, lambda: nm.generate(texts, frames, RtSampling(*SAMPLED), seed=9, trace=True)))
    finally:
        nm.close()


def test_equal_width_predictor(ctx):
    """talker.hidden == predictor.hidden: no mtp projection, the table is built from the groups' bf16 embedding tables and
    k_embed_rowsq does the gather (such a model never takes the fused sampler)"""
    from rho_tts_amd._native_model import RtSampling
    base = config.PRESETS["tiny"]()
    dims = TransformerDims(hidden=base.talker.hidden, layers=2, heads=2, kv_heads=1, head_dim=32, inter=128)
    cfg = dataclasses.replace(base, name="tiny-equal-qkv", predictor=dims)
    assert not cfg.has_mtp_proj
    nm, _ = build(ctx, cfg, max_batch=5)
    try:
        set_voice(nm, make_voice(cfg, True))
        texts, frames = ragged(cfg, 5, seed=13)
        same(*both_routes(nm, lambda: nm.generate(texts, frames, RtSampling(*SAMPLED), seed=21, trace=True)))
    finally:
        nm.close()


def test_the_table_route_drops_one_launch_per_pass(model16):
    """the route is really taken: with per-launch profiling on (eager frames), the decode GEMM launches of predictor passes 2..G-1
    (class 2: four per layer and pass) are one per pass and frame fewer, and the codes are still the same"""
    from rho_tts_amd._native_model import RtSampling
    cfg, nm = model16
    G, layers, F = cfg.n_groups, cfg.predictor.layers, 4
    texts, frames = ragged(cfg, 5, seed=19)
    frames = [F] * len(texts)

    def run():
        nm.profile(True)
        try:
            codes = nm.generate(texts, frames, RtSampling(*SAMPLED), seed=31)
            return codes, nm.profile_read_class(2)[0]
        finally:
            nm.profile(False)
    (codes_off, n_off), (codes_on, n_on) = both_routes(nm, run)
    assert all(torch.equal(a, b) for a, b in zip(codes_off, codes_on))
    assert n_off == F * (G - 2) * 4 * layers
    assert n_on == F * (G - 2) * (4 * layers - 1)
