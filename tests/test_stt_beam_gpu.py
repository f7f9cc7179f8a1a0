"""Beam-search speech-to-text end to end (rt_stt_transcribe_beam): width 1 is the batched greedy call; a clip's ids and score in a
batch are bit for bit what it gets alone; ids equal the float64 oracle's (tests/stt_beam_ref.py) on cases chosen by decisive margin,
and the reported score is the teacher-forced score of those ids.

Measured on an MI355X over the 18 cases of tests/stt_beam_cases.py (the smallest model, weight sets A and B): E = max |device
cumulative score - rescore of the same ids| = 1.85e-5 (2.95e-5 over the three clips at Whisper-tiny dimensions); recorded E = 3e-5,
margin constant 4 E = 1.2e-4.  Every case's decisive margin (tests/stt_beam_cases.py lists them: 5.0e-3 ... 2.0e-1; at Whisper-tiny
dimensions 1.8e-3, 1.3e-2 and 3.6e-3) is at least fifteen times the constant."""
import numpy as np
import pytest

from oracle import whisper as OW
from rho_tts_amd import _native
from rho_tts_amd import stt as S
from tests import stt_beam_cases as K
from tests import stt_beam_ref as R
from tests.test_oracle_whisper import clip
from tests.test_stt_batch_gpu import early_ending_state, ragged_clips

pytestmark = pytest.mark.gpu

SR = K.SR


@pytest.fixture(scope="module")
def ctx():
    c = _native.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def tiny(ctx):
    """The smallest model with weight sets A and B: (cfg, {set: (native model, oracle model)})."""
    cfg = S.tiny_test_config()
    sets = {}
    for name, make in K.STATES.items():
        state = make(cfg)
        sets[name] = (S.NativeSTT(ctx, cfg, {k: v.cuda() for k, v in state.items()}), OW.build(cfg, state))
    yield cfg, sets
    for nat, _ in sets.values():
        nat.close()


def test_width_one_is_the_batched_greedy_call(tiny):
    """The exact link between the two paths: the seven ragged clips (ten windows), ids for ids."""
    cfg, sets = tiny
    nat = sets["A"][0]
    assert all(torch_equal(a, b) for a, b in zip(K.state_a(cfg).values(), early_ending_state(cfg).values()))
    clips = ragged_clips()
    ids, scores = nat.transcribe_ids_beam(clips, SR, 1)
    assert ids == nat.transcribe_ids_batch(clips, SR) and any(ids)
    assert all(np.isfinite(s) and s < 0 for s in scores)
    assert nat.transcribe_ids_beam(clips, SR, 1, max_tokens=15)[0] == nat.transcribe_ids_batch(clips, SR, max_tokens=15)


def torch_equal(a, b):
    import torch
    return torch.equal(a, b)


@pytest.mark.parametrize("B", [2, 5])
def test_a_clip_in_a_batch_is_the_clip_alone(tiny, B):
    """Ten windows: at width 5 a group holds six, so the call runs two groups; the 5.3-s clip is three windows.  Bit for bit: the
    ids and the float32 score."""
    cfg, sets = tiny
    nat = sets["A"][0]
    clips = ragged_clips()
    ids, scores = nat.transcribe_ids_beam(clips, SR, B)
    alone = [nat.transcribe_ids_beam([x], SR, B) for x in clips]
    assert ids == [a[0][0] for a in alone] and scores == [a[1][0] for a in alone]
    back = nat.transcribe_ids_beam(clips[::-1], SR, B)
    assert back[0] == ids[::-1] and back[1] == scores[::-1]
    head, tail = nat.transcribe_ids_beam(clips[:3], SR, B), nat.transcribe_ids_beam(clips[3:], SR, B)
    assert head[0] + tail[0] == ids and head[1] + tail[1] == scores
    cut = nat.transcribe_ids_beam(clips, SR, B, max_tokens=2)        # the cap cuts the ids after decoding: the score is the whole clip's
    assert cut[0] == [i[:2] for i in ids] and cut[1] == scores and any(len(i) > 2 for i in ids)
    # a clip of several windows: ids joined, sum of the windows' cumulative scores / sum of (ids + 1)
    long = clips[5]
    win = cfg.chunk_seconds * SR
    parts = [nat.transcribe_ids_beam([long[k * win:(k + 1) * win]], SR, B) for k in range(3)]
    assert ids[5] == sum((p[0][0] for p in parts), [])
    total = sum(p[1][0] * (len(p[0][0]) + 1) for p in parts) / sum(len(p[0][0]) + 1 for p in parts)
    assert abs(scores[5] - total) <= 1e-6 * max(1.0, abs(total))


def test_ids_and_scores_against_the_oracle(tiny):
    """Every case of tests/stt_beam_cases.py: the ids are the float64 rule's, and the score is rescore(ids) / (n + 1) within
    4 E / (n + 1).  The figures are printed before anything is asserted."""
    cfg, sets = tiny
    budget = R.budget_of(cfg)
    rows = []
    for name, clip_name, B, _, _, _, _ in K.CASES:
        nat, model = sets[name]
        x = K.CLIPS[clip_name]()
        mel = R.window_mels(cfg, x, SR)[0]
        (ids,), (score,) = nat.transcribe_ids_beam([x], SR, B)
        want = R.beam_search(model, cfg, mel, B)
        greedy, _ = OW.greedy(model, cfg, mel)
        ended = len(ids) < budget
        err = abs(score * (len(ids) + 1) - R.rescore(model, cfg, mel, ids, ended))
        rows.append((name, clip_name, B, ids, want, greedy, err))
        print(f"set {name} {clip_name} B={B}: margin {want.margin:.3g} final {want.final_margin:.3g} ids {len(ids)} same {ids == want.ids} "
              f"ended {want.ended} |cumulative - rescore| {err:.3g}")
    print("E measured", max(r[-1] for r in rows), "recorded", K.E, "margin constant", K.MARGIN)
    # the conditions on the kept set
    assert len(rows) >= 6 and {2, 3, 5} <= {r[2] for r in rows}
    assert sum(1 for r in rows if r[4].ids != r[5]) >= 4
    assert sum(1 for r in rows if r[4].ended and len(r[4].ids) < budget) >= 2
    for name, clip_name, B, ids, want, _, err in rows:
        assert want.margin >= K.MARGIN, (name, clip_name, B, want.margin)
        assert ids == want.ids, (name, clip_name, B)
        assert err <= 4 * K.E, (name, clip_name, B, err)       # (score x (n + 1) against rescore: the bound 4 E / (n + 1) on the score)


def test_whisper_tiny_dimensions(ctx):
    """head_dim 64 x 6 heads, 1500 encoder positions, the 51865-wide selection over 15 rows at width 5: alone equals batched, the
    score is the rescore of the ids, and the ids are the oracle's wherever its decisive margin meets the constant."""
    cfg = S.SttConfig(max_new_tokens=8)
    state = S.synthetic_state(cfg, 789)
    nat = S.NativeSTT(ctx, cfg, {k: v.cuda() for k, v in state.items()})
    try:
        clips = [clip(0.8, SR, 0), clip(3.3, SR, 3), clip(9.0, SR, 7)]
        ids, scores = nat.transcribe_ids_beam(clips, SR, 5)
        alone = [nat.transcribe_ids_beam([x], SR, 5) for x in clips]
        assert ids == [a[0][0] for a in alone] and scores == [a[1][0] for a in alone] and all(ids)
        model = OW.build(cfg, state)
        held = 0
        for x, i, s in zip(clips, ids, scores):
            mel = R.window_mels(cfg, x, SR)[0]
            want = R.beam_search(model, cfg, mel, 5)
            err = abs(s * (len(i) + 1) - R.rescore(model, cfg, mel, i, len(i) < R.budget_of(cfg)))
            print(f"margin {want.margin:.3g} ids {len(i)} same {i == want.ids} |cumulative - rescore| {err:.3g}")
            assert err <= 4 * K.E
            if want.margin >= K.MARGIN:
                held += 1
                assert i == want.ids
        assert held >= 1
    finally:
        nat.close()


def test_arguments(ctx):
    cfg = S.tiny_test_config()
    nat = S.NativeSTT(ctx, cfg, {k: v.cuda() for k, v in S.synthetic_state(cfg, 789).items()})
    x = clip(0.4, SR, 1)
    try:
        assert nat.transcribe_ids_beam([], SR, 5) == ([], [])
        for bad in (0, 9):
            with pytest.raises(ValueError):
                nat.transcribe_ids_beam([x], SR, bad)
            xs = [nat._pcm(x)]
            import ctypes as C
            ptrs, lens = (C.c_void_p * 1)(xs[0].data_ptr()), (C.c_int64 * 1)(xs[0].numel())
            toks, n = (C.c_int32 * 12)(), (C.c_int32 * 1)()
            assert nat.lib.rt_stt_transcribe_beam(nat.handle, ptrs, lens, 1, SR, bad, toks, 12, n, None) == _native.RT_ERR_INVALID
        with pytest.raises(ValueError):
            nat.transcribe_ids_beam([x], 10, 2)
        with pytest.raises(ValueError):
            nat.transcribe_ids_beam([x], SR, 2, max_tokens=-1)
        ids, scores = nat.transcribe_ids_beam([x], SR, 8)
        assert len(ids) == len(scores) == 1
    finally:
        nat.close()
    with pytest.raises(ValueError):                  # a closed handle
        nat.transcribe_ids_beam([x], SR, 2)
