"""Conditioning on previous text on the CPU: the restated loop (tests/stt_prompt_ref.py) on the cases of tests/stt_prompt_cases.py -
every recorded round count and margin, and the conditions the cases meet together - the logits pin against transformers' forward,
the history rule branch by branch, the configuration, and the argument rules that need no device."""
import dataclasses
import math

import numpy as np
import pytest
import torch

from oracle import whisper as OW
from rho_tts_amd import stt as S
from rho_tts_amd.validation import history_after_window, prompt_for_window
from tests import stt_beam_ref as R
from tests import stt_lang_cases as L
from tests import stt_prompt_cases as PC
from tests import stt_prompt_ref as P
from tests import stt_seek_cases as SC
from tests import stt_seek_ref as SR

CFG = PC.prompt_test_config()
CAP = P.prompt_cap(CFG)
_MODELS = {}


def model_of(st, cfg=CFG):
    key = (st, cfg.max_new_tokens)
    if key not in _MODELS:
        _MODELS[key] = OW.build(cfg, PC.STATES[st](cfg))
    return _MODELS[key]


@pytest.fixture(scope="module")
def runs():
    """{(set, clip, max_initial, width, run): (reference clip, the unconditioned reference clip)}, computed once."""
    out = {}
    for st, cl, mi, B, per in PC.CASES:
        x = PC.CLIPS[cl]()
        plain = SR.clip_transcribe(model_of(st), CFG, x, PC.SR, B, mi)
        for run in per:
            out[(st, cl, mi, B, run)] = (P.clip_transcribe(model_of(st), CFG, x, PC.SR, B, PC.SOT_PREV, mi, True, PC.run_kwargs(run)["initial_ids"] or []), plain)
    return out


def test_the_configuration():
    assert CAP == 15 and CFG.n_text_ctx == 32 and CFG.vocab == 400
    used = {CFG.eos_id, CFG.no_speech_id, *CFG.prefix, *CFG.languages.values()}
    assert PC.SOT_PREV not in used and CFG.eos_id < PC.SOT_PREV < CFG.timestamp_begin - 1
    assert L.LANGUAGES["ja"] == 294 and L.LANGUAGES["ko"] == PC.SOT_PREV and "ko" not in CFG.languages      # (294 is taken; 295 is freed here)
    assert all(0 <= t < CFG.eos_id for t in PC.INITIAL) and len(PC.INITIAL) == 4


def test_recorded_rounds_and_margins(runs):
    for (st, cl, mi, B, run), (c, _) in runs.items():
        rounds, margin = next(per for s, k, m, b, per in PC.CASES if (s, k, m, b) == (st, cl, mi, B))[run]
        print(f"set {st} {cl} max_initial {mi} B={B} {run}: rounds {len(c.windows)} margin {c.margin:.3g} prompts {[len(w.prompt) for w in c.windows]}")
        assert len(c.windows) == rounds and c.margin >= PC.MARGIN, (st, cl, mi, B, run, len(c.windows), c.margin)
        assert c.margin == pytest.approx(margin, rel=0.02)


def test_the_kept_cases_cover_what_the_issue_asks():
    pairs = {(st, cl, mi, B) for st, cl, mi, per in SC.CASES for B in per}
    kept = {(st, cl, mi, B) for st, cl, mi, B, _ in PC.CASES}
    assert len(pairs) == 16 and kept | set(PC.LEFT_OUT) == pairs and not kept & set(PC.LEFT_OUT) and len(PC.LEFT_OUT) <= 4
    for st in "AB":                                           # both widths remain for at least one clip of each weight set
        assert any((st, cl, mi, 1) in kept and (st, cl, mi, 5) in kept for _, cl, mi, _ in pairs)


def test_left_out_pairs_are_below_the_margin():
    for st, cl, mi, B in PC.LEFT_OUT:
        c = P.clip_transcribe(model_of(st), CFG, PC.CLIPS[cl](), PC.SR, B, PC.SOT_PREV, mi, True, PC.INITIAL)
        assert c.margin < PC.MARGIN, (st, cl, mi, B, c.margin)


def test_conditions_the_cases_meet_together(runs):
    seen = set()
    for (st, cl, mi, B, run), (c, plain) in runs.items():
        hist = list(PC.INITIAL) if run == "initial" else []
        for k, w in enumerate(c.windows):
            assert w.prompt == hist[-CAP:]                    # (no case resets: the history is never cut at a mark)
            if 0 < len(w.prompt) < CAP:
                seen.add("a")
            if len(w.prompt) == CAP and len(hist) > CAP:
                seen.add("b")
            kept = [t for a, b, text, raw in w.slices if a != b and text for t in raw]
            tail = w.ids[sum(len(raw) for _, _, _, raw in w.slices):]
            if k + 1 < len(c.windows):
                nxt = c.windows[k + 1].prompt
                assert nxt == (hist + kept)[-CAP:]
                if tail and kept and (hist + kept + tail)[-CAP:] != nxt:
                    seen.add("c")                             # a discarded tail that would have shown in the next prompt, and does not
                if not tail and w.ids and kept == w.ids and w.advance == CFG.n_timestamps - 1 and nxt[-len(w.ids):] == w.ids:
                    seen.add("d")                            # a window consumed whole: every id of it ends the next prompt
            hist += kept
        assert c.history == hist
        if run == "conditioned" and c.ids != plain.ids:
            seen.add("e")
        if run == "initial" and c.windows[0].ids != plain.windows[0].ids and c.windows[0].prompt == PC.INITIAL:
            seen.add("f")
    assert seen == set("abcdef"), seen


def test_a_binding_budget():
    cfg = PC.budget_config()
    assert cfg.max_new_tokens == 16
    for st, cl, mi, B, rounds, margin, budgets, n_ids in PC.BUDGET_CASES:
        c = P.clip_transcribe(model_of(st, cfg), cfg, PC.CLIPS[cl](), PC.SR, B, PC.SOT_PREV, mi, True, [])
        assert len(c.windows) == rounds and c.margin >= PC.MARGIN and c.margin == pytest.approx(margin, rel=0.02)
        assert [w.budget for w in c.windows] == budgets and [len(w.ids) for w in c.windows] == n_ids
        assert all(w.budget == min(16, 32 - (3 + (1 + len(w.prompt) if w.prompt else 0))) for w in c.windows)
    # (g): one clip's windows stop at both budgets - 16 steps without a prompt, 13 behind a full one
    both = [any(b == 16 == n for b, n in zip(bs, ns)) and any(b == 13 == n for b, n in zip(bs, ns)) for *_, bs, ns in PC.BUDGET_CASES]
    assert sum(both) >= 2


def test_the_prefix_is_what_the_model_forward_sees():
    """Logits behind [sot_prev] + prompt + prefix from the reference helper (encoder states handed over) equal those of
    WhisperForConditionalGeneration's forward on the features and the same decoder ids; the language stays at position 1 of the
    forced part."""
    model = model_of("A")
    x = PC.CLIPS["clip(5.0, 2)"]()[:2 * PC.SR]
    mel = SR.own_features(CFG, x, PC.SR)(0, len(x))
    for prompt, lang in (([], None), ([5, 9], None), (list(range(20, 35)), 294)):
        prefix = P.window_prefix(CFG, PC.SOT_PREV, prompt, lang)
        forced = [291, lang or 292, 296]
        assert prefix == (([PC.SOT_PREV] + prompt) if prompt else []) + forced and len(prefix) <= 19
        assert P.budget_of(CFG, prefix) == min(CFG.max_new_tokens, 32 - len(prefix))
        got = SR._logits(model, R.encode(model, mel), prefix, [[]])[0]
        with torch.no_grad():
            want = model(input_features=mel[None], decoder_input_ids=torch.tensor([prefix])).logits[0, -1].double().numpy()
        assert np.abs(got - want).max() <= 1e-6


def test_prompt_for_window():
    h = list(range(100, 140))
    assert prompt_for_window([], 0, 15) == [] and prompt_for_window(h[:4], 0, 15) == h[:4]
    assert prompt_for_window(h, 0, 15) == h[-15:] and prompt_for_window(h, 30, 15) == h[30:] and prompt_for_window(h, 40, 15) == []
    assert prompt_for_window(h, 20, 15) == h[25:]            # the cap cuts behind the mark, never before it
    assert prompt_for_window(h[:15], 0, 15) == h[:15] and prompt_for_window(h[:16], 0, 15) == h[1:16]


def test_history_after_window():
    T0 = 299
    pair = (10, 40, [7, 8], [309, 7, 8, 339])
    no_duration = (40, 40, [9], [339, 9, 339])
    no_text = (40, 60, [], [339, 359])
    h0 = [1, 2, 3]
    assert history_after_window(h0, 0, [pair, no_duration, no_text, pair]) == (h0 + pair[3] * 2, 0)
    assert history_after_window(h0, 1, [pair], silent=True, condition_on_previous=False) == (h0, 1)          # a silent window changes nothing
    assert history_after_window(h0, 0, [pair], condition_on_previous=False) == (h0 + pair[3], 7)              # conditioning off: the mark moves
    assert history_after_window(h0, 0, [], condition_on_previous=False) == (h0, 3)
    assert history_after_window(h0, 2, [pair], temperature=0.4) == (h0 + pair[3], 2)                          # 0.4 is not above 0.5: kept
    assert history_after_window(h0, 2, [pair], temperature=0.6) == (h0 + pair[3], 7)                          # 0.6 is: dropped
    assert history_after_window(h0, 2, [pair], temperature=0.5) == (h0 + pair[3], 2)
    assert history_after_window(h0, 2, [pair], temperature=1.0, reset_on_temperature=None) == (h0 + pair[3], 2)
    # the slices of the seek rule: a tail behind the last pair is no slice; a window without a pair is one slice of everything
    tailed = [309, 7, 339, 339, 8, 9]
    assert [s[3] for s in P.raw_slices(tailed, T0, 100, 100)] == [[309, 7, 339, 339]]      # (the last slice keeps both timestamps of its pair)
    single = [309, 7, 339, 339, 8, 349]
    assert [s[3] for s in P.raw_slices(single, T0, 100, 100)] == [[309, 7, 339], [339, 8, 349]]
    assert P.raw_slices([309, 7, 8], T0, 80, 100) == [(0, 10, [7, 8], [309, 7, 8])]
    assert P.raw_slices([299], T0, 80, 100) == [(0, 80, [], [299])]


def test_the_configuration_carries_startofprev():
    js = dict(d_model=384, vocab_size=51865)
    assert S.SttConfig().sot_prev_id == 50361 and S.SttConfig.from_hf(js).sot_prev_id == 50361
    gen = dict(prev_sot_token_id=50360, no_timestamps_token_id=50363, lang_to_id={"<|en|>": 50259}, task_to_id={"transcribe": 50359})
    assert S.SttConfig.from_hf(js, gen).sot_prev_id == 50360
    assert S.SttConfig.from_hf(dict(js, vocab_size=51864, decoder_start_token_id=50257)).sot_prev_id is None      # a vocabulary this build does not know
    assert S.tiny_test_config().sot_prev_id is None and CFG.sot_prev_id == PC.SOT_PREV


def test_set_prompt_arguments():
    ok = S.check_prompt_args(CFG, [1, 2], False, 0.5)
    assert ok == ([1, 2], 0.5) and S.check_prompt_args(CFG, None, True, None) == ([], None)
    for cfg, kw in ((CFG, dict(initial_ids=None, condition_on_previous=False)),                       # neither
                    (CFG, dict(initial_ids=[400], condition_on_previous=False)),                       # outside the vocabulary
                    (CFG, dict(initial_ids=[-1], condition_on_previous=True)),
                    (CFG, dict(initial_ids=[1.5], condition_on_previous=True)),
                    (CFG, dict(initial_ids="hello", condition_on_previous=True)),
                    (CFG, dict(initial_ids=None, condition_on_previous=True, reset_on_temperature=-0.1)),
                    (CFG, dict(initial_ids=None, condition_on_previous=True, reset_on_temperature=math.inf)),
                    (dataclasses.replace(CFG, sot_prev_id=None), dict(initial_ids=[1], condition_on_previous=True)),
                    (dataclasses.replace(CFG, sot_prev_id=290), dict(initial_ids=[1], condition_on_previous=True)),
                    (dataclasses.replace(CFG, timestamp_begin=None), dict(initial_ids=[1], condition_on_previous=True))):
        kw.setdefault("reset_on_temperature", 0.5)
        with pytest.raises(ValueError):
            S.check_prompt_args(cfg, **kw)
    closed = object.__new__(S.NativeSTT)
    closed.handle = None
    with pytest.raises(ValueError):
        closed.set_prompt([1], True)


def test_transcriber_arguments():
    for kw in (dict(condition_on_previous_text=True), dict(initial_prompt=[1, 2]), dict(initial_prompt="a name")):
        with pytest.raises(ValueError, match="timestamps=True"):
            S.WhisperTranscriber(None, synthetic=True, cfg=CFG, **kw)
