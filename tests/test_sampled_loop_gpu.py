"""A sampled generation, draw by draw, against the sampler's definition: tests/sampling_ref.py replays a finished
nm.generate(..., trace=True) from the GPU's OWN traced logits - item by item, frame by frame, group by group - and every decided
draw (margin >= 2^-20) must be the code the generation returned; at most 1 % of a case's draws may be undecided.  That pins what
the loop adds to the sampler launch: the key (seed, item id, the item's own frame, group), the penalty history carried over the
frames, the end of sequence admitted from min_frames on and written as a stop.  Each case also shows, with the reference alone,
that it could fail: the replay with frame + 1, item + 1, group + 1, without the history and with the end of sequence allowed from
frame 0 each changes decided draws.  The sampled run's logits are tied to the model oracle through the teacher-forced run of the
same codes (test_teacher_forced_logits_match_oracle ties forced traces to OracleModel).

Each case prints its draws / undecided / smallest decided margin."""
import dataclasses

import pytest
import torch

from rho_tts_amd import config, weights
from tests.sampling_ref import CAP, DECIDED, SamplingParams, replay, tally
from tests.test_model_gpu import make_voice, set_voice

pytestmark = pytest.mark.gpu

SET_A, SET_B = (0.9, 50, 1.0, 1.05), (1.3, 64, 0.8, 1.3)          # (temperature, top_k, top_p, repetition penalty)
HOT = (3.0, 64, 1.0, 1.3)                                          # near-uniform over the top 64: ends of sequence do get drawn
IDS = [5, 0, 2 ** 32 + 9, 3, 2 ** 31 + 1, 17, 8, 2 ** 33 + 2, 40, 41, 42, 43, 44, 45, 46, 47]


def wide_tiny():
    """tiny's topology with the shipped vocabularies: codebook 2048, talker vocabulary 3072 (the 16-wave sampler), predictor
    vocabulary 2048 (the 8-wave one); the control ids move to their shipped places above the codebook."""
    base = config.PRESETS["tiny"]()
    d = config.ModelConfig(name="x", talker=base.talker, predictor=base.predictor)
    ids = {k: getattr(d, k) for k in ("codec_pad_id", "codec_bos_id", "codec_eos_id", "codec_think_id", "codec_nothink_id", "codec_think_bos_id",
                                      "codec_think_eos_id", "language_ids", "speaker_ids")}
    return dataclasses.replace(base, name="tiny-wide", codec=dataclasses.replace(base.codec, codebook_size=2048), codec_vocab=3072,
                               predictor_vocab=2048, **ids)


CONFIGS = {"tiny": config.PRESETS["tiny"], "small": config.PRESETS["small"], "wide": wide_tiny}
PEAKED = {"small": 48, "wide": 48}


def model_state(name, cfg):
    """The synthetic weights of tests/test_model_gpu.py.  With 256 or 2048 codes of equal standing the end of sequence is hardly
    ever among the top 64, and a sampler that admitted it too early would draw the same tokens: for these configurations the talker
    head's rows of all but the first 48 codes are scaled down, so that the distribution is peaked - as a trained model's is - and
    the control id competes."""
    state = weights.synthetic_state(cfg, 789)
    if name in PEAKED:
        state["talker.codec_head.weight"][PEAKED[name]:cfg.codec.codebook_size] *= 0.05
    return state


# name: (config, items, frames per item, talker set, predictor set, min_frames, seed, route: the rt_debug_tune code or None)
ROUTE_BACK = {800: 801, 200: 201, 100: 101, 3100: 3101}          # the code that restores the default route
CASES = {
    "tiny-default": ("tiny", 8, 7, SET_B, SET_A, 2, 11, None),
    "tiny-16-min4": ("tiny", 16, 9, SET_A, SET_B, 4, 12, None),
    "small-default": ("small", 12, 6, SET_A, SET_B, 2, 13, None),
    "small-min4": ("small", 6, 7, SET_B, SET_A, 4, 14, None),
    "tiny-unfused-800": ("tiny", 8, 6, SET_B, SET_A, 2, 15, 800),
    "tiny-eager-200": ("tiny", 8, 6, SET_A, SET_B, 2, 16, 200),
    "small-legacy-100": ("small", 5, 5, SET_B, SET_A, 2, 17, 100),
    "tiny-gemm-3100": ("tiny", 8, 6, SET_B, SET_B, 2, 18, 3100),
    "wide-default": ("wide", 6, 6, SET_B, SET_A, 2, 19, None),
    "tiny-hot": ("tiny", 16, 9, HOT, SET_A, 2, 20, None),
}


def case_inputs(cfg, n, frames, seed):
    g = torch.Generator().manual_seed(seed)
    texts = [[int(v) for v in torch.randint(0, cfg.text_vocab - 64, (int(k),), generator=g)] for k in torch.randint(1, 8, (n,), generator=g)]
    n_frames = [frames - (i % 3 == 1) for i in range(n)]              # ragged limits: every third item one frame shorter
    return texts, n_frames, IDS[:n]


def params(s):
    from rho_tts_amd._native_model import RtSampling
    return SamplingParams(True, *s), RtSampling(1, *s)


@pytest.fixture(scope="module")
def ctx():
    from rho_tts_amd import _native
    c = _native.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def models(ctx):
    """One model per configuration, built at its first use and kept for the module."""
    from rho_tts_amd._native_model import NativeModel
    made = {}

    def get(name):
        if name not in made:
            cfg = CONFIGS[name]()
            nm = NativeModel(ctx, cfg, max_batch=16)
            nm.load_state({k: v.cuda() for k, v in model_state(name, cfg).items()})
            set_voice(nm, make_voice(cfg, True))
            made[name] = (cfg, nm)
        return made[name]
    yield get
    for _, nm in made.values():
        nm.close()


def cpu(tr):
    return {k: v.cpu() for k, v in tr.items()}


def changed(base, other):
    """Decided draws of `base` whose token the other sampler draws differently (same positions; an other replay may hold one draw
    more or fewer only through the end of sequence, which shifts nothing: draws are matched by (item, frame, group))."""
    o = {d[:3]: d[3] for d in other}
    return sum(1 for d in base if d[4] >= DECIDED and d[:3] in o and o[d[:3]] != d[3])


def check_replay(name, cfg, codes, n_frames, tr, sp_t, sp_p, seed, ids, ignore_eos, min_frames, mutations=True, forced_frames=None):
    args = (cfg, codes, n_frames, tr, sp_t, sp_p, seed, ids, ignore_eos, min_frames)
    draws = replay(*args, forced_frames=forced_frames)
    n, undecided, bad, min_margin = tally(draws)
    print(f"{name}: {n} draws, {undecided} undecided, smallest decided margin {min_margin:.3e}, "
          f"{sum(1 for c, f in zip(codes, n_frames) if c.shape[0] < f)} items stopped early")
    assert not bad, f"{name}: decided draws differ (item, frame, group, reference, margin, generation): {bad[:8]}"
    assert undecided <= CAP * n, f"{name}: {undecided} of {n} draws undecided"
    if mutations:             # the reference alone: a sampler with one of these defects would have failed the comparison above
        for what, kw in (("frame + 1", dict(frame_add=1)), ("item + 1", dict(item_add=1)), ("group + 1", dict(group_add=1)),
                         ("no history", dict(history=False)), ("end of sequence from frame 0", dict(eos_from=0))):
            assert changed(draws, replay(*args, **kw)) >= 1, f"{name}: the case cannot tell a sampler with {what} apart"
    return draws


@pytest.mark.parametrize("name", list(CASES))
def test_sampled_generation_replays_draw_by_draw(models, name):
    from rho_tts_amd._native_model import RtSampling
    cfg_name, n, frames, set_t, set_p, min_frames, seed, route = CASES[name]
    cfg, nm = models(cfg_name)
    texts, n_frames, ids = case_inputs(cfg, n, frames, seed)
    (sp_t, rt_t), (sp_p, rt_p) = params(set_t), params(set_p)
    try:
        if route is not None:
            nm.lib.rt_debug_tune(route, 0)
        codes, tr = nm.generate(texts, n_frames, rt_t, rt_p, seed=seed + (3 << 32), item_ids=ids, ignore_eos=False, min_frames=min_frames, trace=True)
        # the same launches with the codes forced under greedy parameters: the logits are those of the sampled run
        greedy = RtSampling(0, 1.0, 1, 1.0, 1.0)
        full = [c.shape[0] == f for c, f in zip(codes, n_frames)]
        assert all(c.shape[0] >= min_frames for c in codes)
        again, tr_f = nm.generate(texts, [c.shape[0] for c in codes], greedy, greedy, forced_codes=codes, trace=True)
    finally:
        if route is not None:
            restore = ROUTE_BACK[route]
            nm.lib.rt_debug_tune(restore, 0)
    tr, tr_f = cpu(tr), cpu(tr_f)
    check_replay(name, cfg, codes, n_frames, tr, sp_t, sp_p, seed + (3 << 32), ids, False, min_frames)
    if name == "tiny-hot":
        assert not all(full), "no item met the end of sequence: the case needs another seed"
    for b, c in enumerate(codes):
        T = c.shape[0]
        assert torch.equal(again[b], c)
        assert torch.equal(tr_f["talker"][:T, b], tr["talker"][:T, b]), (name, b)
        assert torch.equal(tr_f["predictor"][:T, :, b], tr["predictor"][:T, :, b]), (name, b)


@pytest.mark.parametrize("cfg_name", ["tiny", "small"])
def test_forced_end_of_sequence_and_free_greedy_frames(models, cfg_name):
    """A voice-less greedy run as in test_eos_and_max_frames: item 0 is forced to the end of sequence at frame 2 and returns two
    frames; item 1 is forced for three frames and then draws group 0 freely (the other groups stay forced to the last forced frame,
    as in the oracle) - those draws replay as arg-max draws under penalty 1.3, the history counting the forced codes."""
    from rho_tts_amd._native_model import RtSampling
    cfg, nm = models(cfg_name)
    G = cfg.n_groups
    forced = [torch.tensor([[1] * G, [2] * G, [cfg.codec_eos_id] + [0] * (G - 1)]), torch.randint(0, 60, (3, G), generator=torch.Generator().manual_seed(1))]
    try:
        set_voice(nm, make_voice(cfg, False))
        greedy = RtSampling(0, 1.0, 1, 1.0, 1.3)
        codes, tr = nm.generate([[1, 2], [3]], [5, 6], greedy, greedy, item_ids=[9, 2 ** 32 + 1], ignore_eos=False, min_frames=2, forced_codes=forced, trace=True)
    finally:
        set_voice(nm, make_voice(cfg, True))
    assert codes[0].shape[0] == 2 and torch.equal(codes[0], forced[0][:2])
    assert torch.equal(codes[1][:3], forced[1]) and 3 <= codes[1].shape[0] <= 6
    sp = SamplingParams(False, 1.0, 1, 1.0, 1.3)
    draws = check_replay(f"forced-{cfg_name}", cfg, codes, [5, 6], cpu(tr), sp, sp, 789, [9, 2 ** 32 + 1], False, 2, mutations=False, forced_frames=[3, 3])
    assert torch.equal(codes[1][3:, 1:], forced[1][2:3, 1:].expand(codes[1].shape[0] - 3, -1))
    assert len(draws) == codes[1].shape[0] - 3 + (codes[1].shape[0] < 6) >= 1
