"""Decode on 65..128 rows: a text's codes (and waveform) may not depend on what it was batched with, so every item of a wide
batch - static, queued, on fewer rows than the model has - must equal, bit for bit, what it produces alone in a one-item call;
under one 128-row GEMM launch per weight matrix (rt_debug_tune 3201) and under two 64-row launches (3200).

Presets: `tiny`, and `small` with 8 talker KV heads: the stock `small` has 4, so 128 rows x 4 heads still sit on the bound up to
which decode attention takes its 16-wave split and a merge order that changed with the batch width would go unseen.  Both run
with a cloned voice (a shared prefix) and max_positions > 64, so the 16-wave form is what a lone item gets.
"""
import dataclasses

import pytest
import torch

from rho_tts_amd import config
from tests.test_model_gpu import build, make_voice, set_voice

pytestmark = pytest.mark.gpu

ROWS = [0, 15, 16, 63, 64, 65, 79, 80, 111, 112, 119]        # sub-block and 64-row edges of a 120-row batch
LATE = [128, 131, 137, 144, 149]                             # items of a 150-item queue that start at a hand-over
N_STATIC, N_QUEUED = 120, 150


def preset_cfg(name):
    cfg = config.PRESETS[name]()
    if name == "small":
        cfg = dataclasses.replace(cfg, talker=dataclasses.replace(cfg.talker, heads=8, kv_heads=8), max_positions=128)
    return cfg


@pytest.fixture(scope="module")
def ctx():
    from rho_tts_amd import _native
    c = _native.Context(0)
    yield c
    c.close()


class Case:
    """One 128-row model, its work list and the codes each item produces alone (computed once, on demand)."""

    def __init__(self, ctx, name, frames_lo=3, frames_hi=8):
        from rho_tts_amd._native_model import RtSampling
        self.cfg = preset_cfg(name)
        self.nm, _ = build(ctx, self.cfg, max_batch=128)
        set_voice(self.nm, make_voice(self.cfg, True))
        g = torch.Generator().manual_seed(23)
        self.texts = [[int(v) for v in torch.randint(0, self.cfg.text_vocab - 64, (int(k),), generator=g)]
                      for k in torch.randint(1, 7, (N_QUEUED,), generator=g)]
        self.frames = [int(v) for v in torch.randint(frames_lo, frames_hi + 1, (N_QUEUED,), generator=g)]
        self.ids = [50 + 3 * i for i in range(N_QUEUED)]
        self.sp = RtSampling(1, 0.9, 50, 1.0, 1.05)           # sampled, repetition penalty on
        self.live = RtSampling(1, 1.5, 64, 1.0, 1.0)          # hot sampling over the full top-k: end-of-sequence gets drawn
        self._alone, self._alone_live = {}, {}

    def alone(self, i):
        if i not in self._alone:
            self._alone[i] = self.nm.generate([self.texts[i]], [self.frames[i]], self.sp, seed=5, item_ids=[self.ids[i]])[0]
        return self._alone[i]

    def alone_live(self, i):
        if i not in self._alone_live:
            self._alone_live[i] = self.nm.generate([self.texts[i]], [self.frames[i]], self.live, seed=6, item_ids=[self.ids[i]], ignore_eos=False,
                                                   min_frames=2)[0]
        return self._alone_live[i]

    def batch(self, n, **kw):
        return self.nm.generate(self.texts[:n], self.frames[:n], self.sp, seed=5, item_ids=self.ids[:n], **kw)


@pytest.fixture(scope="module", params=["tiny", "small"])
def case(request, ctx):
    c = Case(ctx, request.param)
    yield c
    c.nm.lib.rt_debug_tune(3201, 0)
    c.nm.lib.rt_debug_tune(1704, 0)
    c.nm.close()


def test_max_batch_range(ctx, case):
    """rt_model_create takes 1..128 rows (the fixture's model has 128) and refuses 129 with RT_ERR_INVALID."""
    from rho_tts_amd._native_model import NativeModel
    assert case.nm.max_batch == 128
    with pytest.raises(ValueError):                             # (RT_ERR_INVALID is raised as ValueError)
        NativeModel(ctx, case.cfg, max_batch=129)


@pytest.mark.parametrize("wide", [0, 1])
def test_static_batch_of_120_rows(case, wide):
    case.nm.lib.rt_debug_tune(3200 + wide, 0)
    try:
        got = case.batch(N_STATIC)
        st = case.nm.generate_stats()
    finally:
        case.nm.lib.rt_debug_tune(3201, 0)
    assert st["rows"] == N_STATIC and [c.shape[0] for c in got] == case.frames[:N_STATIC]
    for i in ROWS:
        assert torch.equal(got[i], case.alone(i)), (wide, i)


@pytest.mark.parametrize("wide", [0, 1])
def test_queued_items_on_128_rows(case, wide):
    """150 items on 128 rows: the first 128 start on row = index, the others take over finished rows."""
    n = N_QUEUED
    case.nm.lib.rt_debug_tune(3200 + wide, 0)
    try:
        for every in (4, 1):
            case.nm.lib.rt_debug_tune(1700 + every, 0)
            got = case.batch(n)
            st = case.nm.generate_stats()
            assert st["rows"] == 128 and st["hand_overs"] >= 1 and st["frames_kept"] == sum(case.frames)
            for i in ROWS + LATE:
                assert torch.equal(got[i], case.alone(i)), (wide, every, i)
    finally:
        case.nm.lib.rt_debug_tune(1704, 0)
        case.nm.lib.rt_debug_tune(3201, 0)


def test_queued_items_with_live_end_of_sequence(ctx):
    case = Case(ctx, "tiny", 6, 24)                              # (longer budgets: end-of-sequence has to be drawn inside them)
    try:
        n = N_QUEUED
        got = case.nm.generate(case.texts, case.frames, case.live, seed=6, item_ids=case.ids, ignore_eos=False, min_frames=2)
        assert case.nm.generate_stats()["rows"] == 128
        picked = ROWS + LATE
        assert any(case.alone_live(i).shape[0] < case.frames[i] for i in range(0, n, 3)), "no item ended early: the live case tests nothing"
        for i in picked:
            assert torch.equal(got[i], case.alone_live(i)), i
    finally:
        case.nm.close()


def test_fewer_rows_than_the_model_has_and_narrow_batches_afterwards(case):
    """max_rows = 96 on the 128-row model (a queue on 96 rows), then a 64-row and a 4-row static batch: the graphs captured for
    the wide shapes must not be replayed for them."""
    got = case.batch(N_STATIC, max_rows=96)
    assert case.nm.generate_stats()["rows"] == 96
    for i in ROWS:
        assert torch.equal(got[i], case.alone(i)), i
    wide = case.batch(N_STATIC)                                  # (a 120-row frame in between)
    assert torch.equal(wide[119], case.alone(119))
    got = case.batch(64)
    assert case.nm.generate_stats()["rows"] == 64
    for i in list(range(0, 64, 7)) + [63]:
        assert torch.equal(got[i], case.alone(i)), i
    got = case.batch(4)
    assert case.nm.generate_stats()["rows"] == 4
    for i in range(4):
        assert torch.equal(got[i], case.alone(i)), i


def test_code2wav_of_128_items(ctx):
    """rt_code2wav follows max_batch: 128 short items in one call, each waveform bit-equal to its own one-item call."""
    cfg = preset_cfg("tiny")
    nm, _ = build(ctx, cfg, max_batch=128)
    try:
        g = torch.Generator().manual_seed(31)
        codes = [torch.randint(0, cfg.codec.codebook_size, (int(t), cfg.n_groups), generator=g) for t in torch.randint(2, 9, (128,), generator=g)]
        wavs = [w.clone() for w in nm.code2wav(codes)]
        assert len(wavs) == 128
        for i, c in enumerate(codes):
            one = nm.code2wav([c])[0]
            assert one.numel() > 0 and torch.equal(one, wavs[i]), i
    finally:
        nm.close()
