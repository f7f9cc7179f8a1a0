"""Conditioning on previous text on the GPU (rt_stt_set_prompt) against the float64 restatement (tests/stt_prompt_ref.py) on the cases
of tests/stt_prompt_cases.py, whose margins and conditions tests/test_stt_prompt_cpu.py asserts: ids, segments in ticks, offsets,
advances, prompt lengths and reset flags exact, every window's cumulative log-probability within 4 E.  And: four clips in one call -
prefixes of different lengths and a binding budget in one group - each what it is alone; the fallback interplay; a policy set and
cleared; the transcriber end to end; the argument rules of the library.

Measured on an MI355X (this file prints the figures): see MEASURED in tests/stt_prompt_cases.py."""
import ctypes as C
import dataclasses

import pytest

from oracle import whisper as OW
from rho_tts_amd import _native
from rho_tts_amd import stt as S
from tests import stt_prompt_cases as PC
from tests import stt_prompt_ref as P
from tests import stt_sample_cases as FC
from tests import stt_sample_ref as F
from tests import stt_seek_cases as SC

pytestmark = pytest.mark.gpu

SR_IN = PC.SR
CFG = PC.prompt_test_config()


@pytest.fixture(scope="module")
def ctx():
    c = _native.Context(0)
    yield c
    c.close()


def make(ctx, cfg):
    made = {}
    for name, build in PC.STATES.items():
        state = build(cfg)
        made[name] = (S.NativeSTT(ctx, cfg, {k: v.cuda() for k, v in state.items()}), OW.build(cfg, state))
    return made


@pytest.fixture(scope="module")
def sets(ctx):
    made = make(ctx, CFG)
    yield made
    for nat, _ in made.values():
        nat.close()


@pytest.fixture(scope="module")
def budget_sets(ctx):
    made = make(ctx, PC.budget_config())
    yield made
    for nat, _ in made.values():
        nat.close()


def report(nat, c):
    """What a clip's result is compared by; the reset flags are the report's (one clip to a call)."""
    lines = nat.prompt_report()
    assert [w.prompt_len for w in lines] == [w.prompt_len for w in c.windows]
    return (c.ids, [(g.start_tick, g.end_tick, g.ids) for g in c.segments], [(w.offset, w.n_ids, w.advance, w.prompt_len) for w in c.windows], [w.reset for w in lines])


def ref_report(c):
    return (c.ids, [(a, b, t) for a, b, t in c.segments], [(w.offset, len(w.ids), w.advance, len(w.prompt)) for w in c.windows], [w.reset for w in c.windows])


@pytest.mark.parametrize("run", ["conditioned", "initial"])
@pytest.mark.parametrize("st", ["A", "B"])
def test_cases_against_the_reference(sets, st, run):
    nat, model = sets[st]
    worst = 0.0
    try:
        for s_, cl, mi, B, per in PC.CASES:
            if s_ != st:
                continue
            x = PC.CLIPS[cl]()
            init = PC.run_kwargs(run)["initial_ids"]
            nat.set_prompt(init, condition_on_previous=True)
            got, = nat.transcribe_ids_seek([x], SR_IN, B, max_initial_timestamp_index=mi, no_speech=False)
            want = P.clip_transcribe(model, CFG, x, SR_IN, B, PC.SOT_PREV, mi, True, init or [])
            errs = [abs(g.logprob - w.logprob) for g, w in zip(got.windows, want.windows)]
            worst = max([worst] + errs)
            same = report(nat, got) == ref_report(want)
            print(f"set {st} {cl} max_initial {mi} B={B} {run}: rounds {len(got.windows)} margin {want.margin:.3g} same {same} prompts {[w.prompt_len for w in got.windows]} "
                  f"max |window logprob - reference| {max(errs):.3g}")
            assert want.margin >= PC.MARGIN and len(want.windows) == per[run][0]
            assert report(nat, got) == ref_report(want), (st, cl, mi, B, run)
            assert max(errs) <= 4 * PC.E and abs(got.score - want.score) <= 4 * PC.E, (st, cl, mi, B, run, errs)
    finally:
        nat.set_prompt(None)
    print("E measured", worst, "recorded", PC.E, "bound", 4 * PC.E)


def test_budget_cases_and_four_clips_at_once(budget_sets):
    """max_new_tokens 16: a window behind a full prompt stops at 13 steps while the others of its group go on to 16.  The cases
    against the reference, then four clips of different lengths in one call - one group holds prefixes of different lengths and
    the binding budget - each bit for bit what it is alone."""
    cfg = PC.budget_config()
    worst = 0.0
    try:
        for st, cl, mi, B, rounds, margin, budgets, n_ids in PC.BUDGET_CASES:
            nat, model = budget_sets[st]
            nat.set_prompt(None, condition_on_previous=True)
            x = PC.CLIPS[cl]()
            got, = nat.transcribe_ids_seek([x], SR_IN, B, max_initial_timestamp_index=mi, no_speech=False)
            want = P.clip_transcribe(model, cfg, x, SR_IN, B, PC.SOT_PREV, mi, True, [])
            errs = [abs(g.logprob - w.logprob) for g, w in zip(got.windows, want.windows)]
            worst = max([worst] + errs)
            print(f"set {st} {cl} max_initial {mi} B={B} max_new 16: n_ids {[w.n_ids for w in got.windows]} prompts {[w.prompt_len for w in got.windows]} "
                  f"max |window logprob - reference| {max(errs):.3g}")
            assert [w.n_ids for w in got.windows] == n_ids and [w.budget for w in want.windows] == budgets
            assert report(nat, got) == ref_report(want), (st, cl, mi, B)
            assert max(errs) <= 4 * PC.E, (st, cl, mi, B, errs)
        print("E measured (budget cases)", worst)
        nat = budget_sets["B"][0]
        # (on the CPU reference, width 1: round 2 holds prompts of 11, 15, 12 and 11 ids and budgets 16 and 13; width 5: rounds 1 to 3 do)
        clips = [PC.CLIPS[k]() for k in ("clip(6.3, 11)", "clip(5.0, 2)", "clip(7.0, 3)", "clip(4.1, 5)")]
        for B in (1, 5):
            nat.set_prompt(None, condition_on_previous=True)
            both = nat.transcribe_ids_seek(clips, SR_IN, B, max_initial_timestamp_index=-1)
            lines = nat.prompt_report()
            alone, alone_lines = [], []
            for x in clips:
                alone.append(nat.transcribe_ids_seek([x], SR_IN, B, max_initial_timestamp_index=-1)[0])
                alone_lines += nat.prompt_report()
            assert both == alone and lines == alone_lines
            assert nat.transcribe_ids_seek(clips[::-1], SR_IN, B, max_initial_timestamp_index=-1) == both[::-1]
            # the uniform gather (the A/B of the ranged one) in this group of short and long prefixes: cut at the cache's end, the same bits
            try:
                assert nat.lib.rt_debug_tune(3300, 0) == 0
                assert nat.transcribe_ids_seek(clips, SR_IN, B, max_initial_timestamp_index=-1) == both
            finally:
                assert nat.lib.rt_debug_tune(3301, 0) == 0
            # a round of this call held prompts of different lengths, and a window that stopped at 13 steps beside one that went on
            by_round = [[c.windows[k] for c in both if k < len(c.windows)] for k in range(max(len(c.windows) for c in both))]
            assert any(len({w.prompt_len for w in r}) >= 2 for r in by_round)
            assert any(any(w.prompt_len == 15 and w.n_ids == 13 for w in r) and any(w.n_ids > 13 for w in r) for r in by_round), [[(w.prompt_len, w.n_ids) for w in r] for r in by_round]
    finally:
        for nat, _ in budget_sets.values():
            nat.set_prompt(None)


class Script:
    """A scripted ratio callback: the given values in call order (1.0 when they run out)."""

    def __init__(self, returns=()):
        self.returns, self.calls = list(returns), 0

        def fn(p_ids, n, _user):
            self.calls += 1
            return float(self.returns[self.calls - 1]) if self.calls <= len(self.returns) else 1.0
        self.cb = S.RATIO_FN(fn)


@pytest.mark.parametrize("B", [1, 5])
def test_fallback_interplay(sets, B):
    """The script fails one attempt of the second window (it stands at temperature 0.2) and three of the third (0.6).  Every attempt of
    a window decodes behind the window's prefix - the sampled ids are those of the restated loop behind that prefix - and the fourth
    window's prompt is empty because 0.6 is above the reset temperature, while the third's is not because 0.2 is below."""
    o = PC.FALLBACK_CASE
    nat, model = sets[o["set"]]
    x = PC.CLIPS[o["clip"]]()
    nt = len(o["temperatures"])
    try:
        s = Script(F.script([[k] for k in o["fails"]], nt))
        nat.set_fallback(o["temperatures"], o["best_of"], logprob_threshold=None, seed=o["seed"], ratio=s.cb)
        nat.set_prompt(None, condition_on_previous=True, reset_on_temperature=0.5)
        got, = nat.transcribe_ids_seek([x], SR_IN, B, max_initial_timestamp_index=o["max_initial"], no_speech=False)
        fb, lines = nat.fallback_report(), nat.prompt_report()
        ret = iter(F.script([[k] for k in o["fails"]], nt))
        pol = P.Policy(o["temperatures"], o["best_of"], o["seed"], lambda ids: next(ret, 1.0), 2.4, None)
        want = P.clip_transcribe(model, CFG, x, SR_IN, B, PC.SOT_PREV, o["max_initial"], True, [], 0.5, None, pol)
        assert all(F.decisive(w.fb, FC.E, FC.G, FC.MARGIN) for w in want.windows)
        assert [w.temperature for w in want.windows] == o["chosen"] and [len(w.prompt) for w in want.windows] == o["prompts"]
        assert [w.temperature for w in fb] == pytest.approx(o["chosen"]) and [w.attempts for w in fb] == o["attempts"]
        assert [w.prompt_len for w in lines] == o["prompts"] and [w.reset for w in lines] == o["reset"]
        for k in range(len(lines) - 1):                       # the next window's prompt is empty exactly when the chosen temperature exceeds 0.5
            assert (lines[k + 1].prompt_len == 0) == (fb[k].temperature > 0.5)
        assert report(nat, got) == ref_report(want)
        errs = [abs(g.logprob - w.logprob) for g, w in zip(got.windows, want.windows)]
        print(f"B={B}: chosen {[w.temperature for w in fb]} prompts {[w.prompt_len for w in lines]} max |window logprob - reference| {max(errs):.3g}")
        assert max(errs) <= 4 * PC.E
    finally:
        nat.set_fallback(None)
        nat.set_prompt(None)


def test_set_then_clear(ctx, sets):
    """A policy set and then cleared: the existing seek cases return ids, segments and scores bit-equal to a handle on which none was
    ever set (the dataclasses compare float32 scores and times)."""
    fresh = S.NativeSTT(ctx, CFG, {k: v.cuda() for k, v in PC.STATES["B"](CFG).items()})
    try:
        nat = sets["B"][0]
        nat.set_prompt(PC.INITIAL, condition_on_previous=True)
        x = PC.CLIPS["clip(5.0, 2)"]()
        with_policy, = nat.transcribe_ids_seek([x], SR_IN, 5, max_initial_timestamp_index=25)
        nat.set_prompt(None)
        assert nat.prompt_report() != [] and not nat._prompt_set
        differs = False
        for st, cl, mi, per in SC.CASES:
            x = SC.CLIPS[cl]()
            for B in per:
                a, = nat.transcribe_ids_seek([x], SR_IN, B, max_initial_timestamp_index=mi)
                b, = fresh.transcribe_ids_seek([x], SR_IN, B, max_initial_timestamp_index=mi)
                assert a == b and all(w.prompt_len == 0 for w in a.windows), (cl, mi, B)
                differs = differs or (cl, mi, B) == ("clip(5.0, 2)", 25, 5) and a != with_policy
        assert differs and nat.prompt_report() == []          # (a call without a policy leaves no report)
        clips = [SC.CLIPS[k]() for k in ("clip(5.0, 2)", "clip(4.1, 5)")]
        assert nat.transcribe_ids_ex(clips, SR_IN, 5) == fresh.transcribe_ids_ex(clips, SR_IN, 5)
        assert nat.transcribe_ids_beam(clips, SR_IN, 5) == fresh.transcribe_ids_beam(clips, SR_IN, 5)
    finally:
        fresh.close()
        sets["B"][0].set_prompt(None)


def test_the_transcriber_conditions_on_previous_text(ctx):
    cfg = dataclasses.replace(CFG, max_initial_timestamp_index=25)
    with pytest.raises(ValueError):                           # a model without a tokenizer takes ids, not a string
        S.WhisperTranscriber(ctx, synthetic=True, cfg=cfg, timestamps=True, initial_prompt="a name")
    empty = S.WhisperTranscriber(ctx, synthetic=True, cfg=cfg, timestamps=True, initial_prompt=[])      # an empty prompt without conditioning: no policy
    try:
        assert not empty.prompted and not empty.model._prompt_set
    finally:
        empty.close()
    t = S.WhisperTranscriber(ctx, synthetic=True, cfg=cfg, timestamps=True, beam_size=5, condition_on_previous_text=True, initial_prompt=PC.INITIAL)
    plain = S.WhisperTranscriber(ctx, synthetic=True, cfg=cfg, timestamps=True, beam_size=5)
    try:
        x = PC.CLIPS["clip(5.0, 2)"]()
        want, = t.model.transcribe_ids_seek([x], SR_IN, 5)
        segs, = t.batch_segments([x], SR_IN)
        assert [(g.start_tick, g.end_tick, g.ids) for g in segs] == [(g.start_tick, g.end_tick, g.ids) for g in want.segments]
        assert [g.text for g in segs] == [" ".join(f"<{i}>" for i in g.ids) for g in want.segments]
        lens = [w.prompt_len for w in want.windows]
        assert lens[0] == len(PC.INITIAL) and max(lens) > lens[0] and {g.prompt_len for g in segs} <= set(lens) and segs[0].prompt_len == lens[0]
        detail, = t.batch_detailed([x], SR_IN)
        assert detail.prompt_len == lens and detail.ids == want.ids and t(x, SR_IN) == detail.text
        other, = plain.batch_detailed([x], SR_IN)
        assert other.prompt_len == [] and other.ids != detail.ids
    finally:
        t.close()
        plain.close()


def test_arguments_of_the_library(ctx, sets):
    nat = sets["A"][0]
    nan = float("nan")

    def call(handle=None, **kw):
        p = S.RtSttPrompt()
        p.sot_prev_id, p.condition_on_previous, p.reset_on_temperature = kw.get("sot", PC.SOT_PREV), kw.get("cond", 1), kw.get("reset", 0.5)
        ids = kw.get("ids", [])
        arr = (C.c_int32 * max(len(ids), 1))(*ids)
        if ids:
            p.h_initial, p.n_initial = arr, len(ids)
        return nat.lib.rt_stt_set_prompt(handle or nat.handle, C.byref(p))
    x = PC.CLIPS["clip(5.0, 2)"]()
    try:
        nat.set_prompt(PC.INITIAL, condition_on_previous=True)
        before, = nat.transcribe_ids_seek([x], SR_IN, 1, max_initial_timestamp_index=25)
        for bad in (dict(sot=CFG.vocab), dict(sot=-1), dict(sot=CFG.eos_id - 1), dict(ids=[CFG.vocab]), dict(ids=[-1]), dict(reset=-0.5), dict(reset=float("inf")),
                    dict(cond=0, ids=[])):
            assert call(**bad) == _native.RT_ERR_INVALID, bad
        assert nat.transcribe_ids_seek([x], SR_IN, 1, max_initial_timestamp_index=25) == [before]      # the policy is unchanged
        assert call(reset=nan) == _native.RT_OK and call(cond=0, ids=[5]) == _native.RT_OK
        bare = S.NativeSTT(ctx, dataclasses.replace(CFG, timestamp_begin=None), {k: v.cuda() for k, v in PC.STATES["A"](CFG).items()})
        try:
            assert call(bare.handle) == _native.RT_ERR_INVALID                                          # a handle without rt_stt_set_timestamps
            with pytest.raises(ValueError):
                bare.set_prompt([1], True)
        finally:
            bare.close()
        n = C.c_int32()
        nat.set_prompt(None, condition_on_previous=True)
        got, = nat.transcribe_ids_seek([x], SR_IN, 1, max_initial_timestamp_index=25)
        lens = (C.c_int32 * 8)(*[-7] * 8)
        assert nat.lib.rt_stt_prompt_report(nat.handle, 1, lens, None, C.byref(n)) == _native.RT_ERR_LENGTH and n.value == len(got.windows) > 1
        assert list(lens)[1:] == [-7] * 7 and lens[0] == 0
        assert nat.lib.rt_stt_prompt_report(nat.handle, 8, lens, None, None) == _native.RT_ERR_INVALID
    finally:
        nat.set_prompt(None)
