"""The temperature fallback on the GPU (rt_stt_set_fallback) against the restated loop (tests/stt_sample_ref.py) on the cases of
tests/stt_sample_cases.py, whose margins tests/test_stt_fallback_cpu.py asserts: attempts, chosen temperature and ids exact, scores
within 4 E.  Ratio decisions come from scripted callbacks, so they have no margin.  And: no policy and a cleared policy return the
bits of before; a clip in a batch is the clip alone; seeds; the seek path; the argument rules; Whisper-tiny dimensions."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

from oracle import whisper as OW
from rho_tts_amd import _native
from rho_tts_amd import stt as S
from tests import stt_beam_cases as K
from tests import stt_beam_ref as R
from tests import stt_sample_cases as FC
from tests import stt_sample_ref as F
from tests import stt_seek_cases as SC
from tests.test_oracle_whisper import clip

pytestmark = pytest.mark.gpu

SR_IN = FC.SR
TICK = int(0.02 * SR_IN)
CFG = FC.CFG
NT = len(FC.TEMPS)


@pytest.fixture(scope="module")
def ctx():
    c = _native.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def setA(ctx):
    state = FC.STATES["A"](CFG)
    nat = S.NativeSTT(ctx, CFG, {k: v.cuda() for k, v in state.items()})
    yield nat, OW.build(CFG, state)
    nat.close()


@pytest.fixture(autouse=True)
def no_policy(setA):
    """Every test starts and ends without a policy on the shared model, whatever the test before it left."""
    setA[0].set_fallback(None)
    yield
    setA[0].set_fallback(None)


def lines(rep):
    """A report as comparable tuples (a NaN ratio - no callback - as None)."""
    return [(w.attempts, w.temperature, None if np.isnan(w.compression_ratio) else w.compression_ratio) for w in rep]


class Script:
    """A scripted ratio callback: returns the given values in call order (1.0 when they run out) and counts its calls."""

    def __init__(self, returns=()):
        self.returns, self.calls, self.seen = list(returns), 0, []

        def fn(p_ids, n, _user):
            self.seen.append([int(p_ids[i]) for i in range(n)])
            self.calls += 1
            return float(self.returns[self.calls - 1]) if self.calls <= len(self.returns) else 1.0
        self.cb = S.RATIO_FN(fn)


def policy(nat, script=None, temps=FC.TEMPS, **kw):
    kw.setdefault("logprob_threshold", None)
    kw.setdefault("compression_ratio_threshold", 2.4 if script is not None else None)
    nat.set_fallback(temps, FC.BEST_OF, seed=kw.pop("seed", FC.SEED), ratio=script.cb if script is not None else None, **kw)


def ragged():
    return [clip(0.4, SR_IN, 1), SC.CLIPS["clip(5.0, 2)"](), K.CLIPS["clip(1.3, 3)"](), SC.CLIPS["clip(4.1, 5)"](), np.zeros(int(0.7 * SR_IN), dtype=np.float32)]


def both_calls(nat, clips, B=FC.BEAM):
    return nat.transcribe_ids_ex(clips, SR_IN, B), nat.transcribe_ids_seek(clips, SR_IN, B, max_initial_timestamp_index=25)


def test_no_policy_and_a_cleared_policy_are_the_bits_of_before(setA):
    nat, _ = setA
    clips = ragged()
    nat.set_fallback(None)
    before = both_calls(nat, clips)
    assert both_calls(nat, clips) == before and nat.fallback_report() == []
    s = Script([9.0] * 64)
    policy(nat, s)
    both_calls(nat, clips)
    rep = nat.fallback_report()                                      # (of the seek call)
    # every window failed every temperature - or its chosen attempt has no text ids: ratio 0, the callback is not asked
    assert s.calls > 0 and all((w.attempts, w.compression_ratio) == (NT, 9.0) or w.compression_ratio == 0.0 for w in rep)
    assert sum(w.attempts == NT for w in rep) >= 3
    nat.set_fallback(None)
    assert both_calls(nat, clips) == before
    # a policy that never triggers: thresholds off, or a scripted ratio of 1.0 throughout - the same bits, one attempt everywhere
    for s in (None, Script()):
        policy(nat, s)
        ex = nat.transcribe_ids_ex(clips, SR_IN, FC.BEAM)
        rep = nat.fallback_report()
        assert ex == before[0] and len(rep) == sum(len(c.windows) for c in ex) and all(w.attempts == 1 and w.temperature == 0.0 for w in rep)
        assert all(np.isnan(w.compression_ratio) if s is None else w.compression_ratio == 1.0 for w in rep)
        assert nat.transcribe_ids_seek(clips, SR_IN, FC.BEAM, max_initial_timestamp_index=25) == before[1]
        assert all(w.attempts == 1 for w in nat.fallback_report())
    # a callback without a compression threshold decides nothing and fills the report
    s = Script([9.0] * 64)
    policy(nat, s, compression_ratio_threshold=None)
    assert nat.transcribe_ids_ex(clips, SR_IN, FC.BEAM) == before[0] and s.calls > 0
    assert all((w.attempts, w.compression_ratio) in ((1, 9.0), (1, 0.0)) for w in nat.fallback_report())
    nat.set_fallback(None)


def ex_reference(model, x, ks, **kw):
    mel = R.window_mels(CFG, x, SR_IN)[0]
    ret = iter(F.script([[ks]], NT) if ks is not None else [])
    return F.window_fallback(model, CFG, mel, FC.BEAM, FC.BEST_OF, FC.TEMPS, FC.SEED, 0, ratio=(lambda ids: next(ret)) if ks is not None else None,
                             **{"logprob_threshold": None, **kw})


@pytest.mark.parametrize("ks", [[1, 0, 2, 3], [2, 3, 1, 1], [3, 1, 0, 2]])
def test_a_scripted_ratio_against_the_restated_loop(setA, ks):
    """Four one-window clips in one group; window w's first ks[w] attempts get ratio 9.0, the next 1.0.  ks[w] == 3: every temperature
    failed, and the choice is the attempt with the largest average."""
    nat, model = setA
    clips = [K.CLIPS[c[1]]() for c in FC.EX_CASES]
    s = Script(F.script([ks], NT))
    policy(nat, s)
    got = nat.transcribe_ids_ex(clips, SR_IN, FC.BEAM)
    rep = nat.fallback_report()
    nat.set_fallback(None)
    assert s.calls == len(s.returns) and len(rep) == len(clips)
    worst = 0.0
    for x, k, g, line in zip(clips, ks, got, rep):
        want = ex_reference(model, x, k)
        assert F.decisive(want, FC.E, FC.G, FC.MARGIN)
        a = want.result
        assert (line.attempts, line.temperature) == (len(want.attempts), pytest.approx(a.temperature)) and g.ids == a.ids, (k, line, a)
        assert line.attempts == min(k + 1, NT) and line.compression_ratio == (9.0 if k == NT else 1.0)
        worst = max(worst, abs(g.windows[0].logprob - a.score))
        assert abs(g.windows[0].logprob - a.score) <= 4 * FC.E and abs(g.score - a.avg) <= 4 * FC.E
    print("max |window logprob - reference|", worst)


def test_a_logprob_threshold_triggers_the_fallback(setA):
    nat, model = setA
    o = FC.LOGPROB_CASE
    x = K.CLIPS[o["clip"]]()
    for thr, attempts in ((o["passes"], 1), (o["fails"], NT)):
        policy(nat, None, logprob_threshold=thr)
        got, = nat.transcribe_ids_ex([x], SR_IN, FC.BEAM)
        line, = nat.fallback_report()
        want = ex_reference(model, x, None, logprob_threshold=thr)
        assert F.decisive(want, FC.E, FC.G, FC.MARGIN) and len(want.attempts) == attempts
        assert (line.attempts, line.temperature, got.ids) == (attempts, pytest.approx(want.result.temperature), want.result.ids) and np.isnan(line.compression_ratio)
        assert abs(got.windows[0].logprob - want.result.score) <= 4 * FC.E
    nat.set_fallback(None)


def test_the_silence_exemption(setA):
    """The clip of zeros with languages set: its average is far below the threshold, so it falls back - unless its no-speech
    probability is above the policy's threshold, which leaves the window to the caller's silence rule."""
    nat, _ = setA
    x = np.zeros(int(0.7 * SR_IN), dtype=np.float32)
    plain, = nat.transcribe_ids_ex([x], SR_IN, FC.BEAM)
    ns, avg = plain.windows[0].no_speech_prob, plain.windows[0].avg_logprob
    assert ns > 0.001 and avg < -1.0
    policy(nat, None, logprob_threshold=-1.0, no_speech_threshold=0.001)
    assert nat.transcribe_ids_ex([x], SR_IN, FC.BEAM) == [plain] and [w.attempts for w in nat.fallback_report()] == [1]
    assert nat.transcribe_ids_ex([x], SR_IN, FC.BEAM, no_speech=False)[0].ids == plain.ids          # (the policy asks for the probe itself)
    assert [w.attempts for w in nat.fallback_report()] == [1]
    policy(nat, None, logprob_threshold=-1.0, no_speech_threshold=min(0.99, 2 * ns + 0.1))
    nat.transcribe_ids_ex([x], SR_IN, FC.BEAM)
    assert [w.attempts for w in nat.fallback_report()] == [NT]
    nat.set_fallback(None)


@pytest.mark.parametrize("temps", [FC.TEMPS, (0.4, 0.8)])
def test_a_clip_in_a_batch_is_the_clip_alone_and_the_seed_decides(setA, temps):
    """Beam 5 and best_of 5: six windows to a group, so the five clips' windows span several groups.  With (0, 0.4, 0.8) every window
    fails every temperature (threshold -1 on averages near -4); with (0.4, 0.8) and no threshold the first, sampled, attempt stands."""
    nat, _ = setA
    clips = ragged()
    thr = -1.0 if temps[0] == 0.0 else None

    def run(xs, seed=FC.SEED):
        policy(nat, None, temps=temps, logprob_threshold=thr, seed=seed)
        ex = nat.transcribe_ids_ex(xs, SR_IN, FC.BEAM)
        rep_ex = nat.fallback_report()
        sk = nat.transcribe_ids_seek(xs, SR_IN, FC.BEAM, max_initial_timestamp_index=25)
        return ex, lines(rep_ex), sk, lines(nat.fallback_report())
    both = run(clips)
    assert sum(len(c.windows) for c in both[0]) > 32 // 5 and len(both[1]) == sum(len(c.windows) for c in both[0])
    assert len(both[3]) == sum(len(c.windows) for c in both[2])
    at_ex = at_sk = 0
    for i, x in enumerate(clips):
        ex, rep_ex, sk, rep_sk = run([x])
        n_ex, n_sk = len(ex[0].windows), len(sk[0].windows)
        assert ex[0] == both[0][i] and rep_ex == both[1][at_ex:at_ex + n_ex] and sk[0] == both[2][i] and rep_sk == both[3][at_sk:at_sk + n_sk]
        at_ex, at_sk = at_ex + n_ex, at_sk + n_sk
    assert run(clips) == both                                        # the same seed: the same bits
    attempts = {w[0] for w in both[1]}
    assert attempts == ({NT} if thr is not None else {1}) and (thr is not None or all(w[1] == pytest.approx(0.4) for w in both[1]))
    if thr is None:                                                  # every window's result is a sampled one: another seed changes some
        other = run(clips, seed=FC.SEED + 1)
        assert [c.ids for c in other[0]] != [c.ids for c in both[0]] and [c.ids for c in other[2]] != [c.ids for c in both[2]]
    nat.set_fallback(None)


@pytest.mark.parametrize("B", [1, 5])
def test_seek_follows_the_chosen_attempt(setA, B):
    nat, model = setA
    st, cl, mi, plain_offsets, offsets = FC.SEEK_CASE
    x = SC.CLIPS[cl]()
    plain, = nat.transcribe_ids_seek([x], SR_IN, B, max_initial_timestamp_index=mi, no_speech=False)
    s = Script([1.0, 9.0])                                           # the second call - the middle window's first attempt - fails
    policy(nat, s)
    got, = nat.transcribe_ids_seek([x], SR_IN, B, max_initial_timestamp_index=mi, no_speech=False)
    rep = nat.fallback_report()
    nat.set_fallback(None)
    ret = iter([1.0, 9.0] + [1.0] * 16)
    want = F.clip_fallback_seek(model, CFG, x, SR_IN, B, FC.BEST_OF, FC.TEMPS, FC.SEED, lambda ids: next(ret), mi, logprob_threshold=None)
    assert all(F.decisive(w.fb, FC.E, FC.G, FC.MARGIN) for w in want)
    assert [w.offset // TICK for w in plain.windows] == plain_offsets and [w.offset // TICK for w in want] == offsets
    assert [(w.offset, w.n_ids, w.advance) for w in got.windows] == [(w.offset, len(w.fb.result.ids), w.advance) for w in want]
    assert [(g.start_tick, g.end_tick, g.ids) for g in got.segments] == [seg for w in want for seg in w.segments]
    assert [(w.attempts, w.temperature) for w in rep] == [(len(w.fb.attempts), pytest.approx(w.fb.result.temperature)) for w in want]
    assert [w.attempts for w in rep] == [1, 2, 1] and s.calls == 4
    assert max(abs(g.logprob - w.fb.result.score) for g, w in zip(got.windows, want)) <= 4 * FC.E
    assert all(t < CFG.timestamp_begin for ids in s.seen for t in ids)          # the callback sees text ids alone


@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("case", range(len(FC.SEEK_SCRIPTS)))
def test_seek_under_scripts_of_two_and_of_every_failed_attempt(setA, case, B):
    """k = 2 and k = n_temperatures through rt_stt_transcribe_seek: the attempt at temperature index 2, and the all-failed choice on
    text ids with the timestamps stripped, each handed to the seek rule - ids, segments, offsets, advances and the report are the
    restated loop's."""
    nat, model = setA
    cl, ks, per = FC.SEEK_SCRIPTS[case]
    offsets, attempts, chosen = per[B]
    x = SC.CLIPS[cl]()
    returns = F.script([[k] for k in ks], NT)
    s = Script(returns)
    policy(nat, s)
    got, = nat.transcribe_ids_seek([x], SR_IN, B, max_initial_timestamp_index=FC.SEEK_MAX_INITIAL, no_speech=False)
    rep = nat.fallback_report()
    nat.set_fallback(None)
    ret = iter(returns + [1.0] * 16)
    want = F.clip_fallback_seek(model, CFG, x, SR_IN, B, FC.BEST_OF, FC.TEMPS, FC.SEED, lambda ids: next(ret), FC.SEEK_MAX_INITIAL, logprob_threshold=None)
    assert all(F.decisive(w.fb, FC.E, FC.G, FC.MARGIN) for w in want)
    assert ([w.offset // TICK for w in want], [len(w.fb.attempts) for w in want], [w.fb.chosen for w in want]) == (offsets, attempts, chosen)
    assert [(w.offset, w.n_ids, w.advance) for w in got.windows] == [(w.offset, len(w.fb.result.ids), w.advance) for w in want]
    assert [(g.start_tick, g.end_tick, g.ids) for g in got.segments] == [seg for w in want for seg in w.segments]
    assert got.ids == [t for w in want for _, _, ids in w.segments for t in ids]
    assert [(w.attempts, w.temperature, w.compression_ratio) for w in rep] == \
        [(len(w.fb.attempts), pytest.approx(w.fb.result.temperature), w.fb.result.ratio) for w in want]
    assert s.calls == sum(attempts) and all(ids and all(t < CFG.timestamp_begin for t in ids) for ids in s.seen)
    assert max(abs(g.logprob - w.fb.result.score) for g, w in zip(got.windows, want)) <= 4 * FC.E


def raw_set(nat, **kw):
    f = S.RtSttFallback()
    f.n_temperatures, f.best_of, f.seed = 2, 5, 1
    f.temperatures[0], f.temperatures[1] = 0.0, 0.5
    f.compression_ratio_threshold = f.logprob_threshold = f.no_speech_threshold = float("nan")
    for k, v in kw.items():
        if k == "temperatures":
            for i, t in enumerate(v):
                f.temperatures[i] = t
        else:
            setattr(f, k, v)
    return nat.lib.rt_stt_set_fallback(nat.handle, C.byref(f))


def test_arguments(ctx, setA):
    nat, _ = setA
    x = K.CLIPS["clip(1.3, 3)"]()
    nat.set_fallback(None)
    good, = nat.transcribe_ids_ex([x], SR_IN, FC.BEAM)
    INV = _native.RT_ERR_INVALID
    assert raw_set(nat) == _native.RT_OK
    nat.set_fallback(None)
    for bad in (dict(n_temperatures=0), dict(n_temperatures=9), dict(best_of=0), dict(best_of=9), dict(temperatures=[0.5, 0.5]), dict(temperatures=[0.5, 0.2]),
                dict(temperatures=[-0.1, 0.2]), dict(temperatures=[0.0, float("nan")]), dict(compression_ratio_threshold=2.4)):
        assert raw_set(nat, **bad) == INV, bad
        assert nat.transcribe_ids_ex([x], SR_IN, FC.BEAM) == [good] and nat.fallback_report() == []          # no policy was set; the handle answers
    for bad in (dict(temperatures=(0.2, 0.1)), dict(temperatures=()), dict(temperatures=(0.0,), best_of=0)):
        with pytest.raises(ValueError):
            nat.set_fallback(**bad)
    # a no_speech_threshold on a handle without languages
    bare = S.NativeSTT(ctx, dataclasses.replace(CFG, languages={}), {k: v.cuda() for k, v in FC.STATES["A"](CFG).items()})
    try:
        assert raw_set(bare, no_speech_threshold=0.6) == INV and raw_set(bare) == _native.RT_OK
        bare.set_fallback(None)
        assert bare.transcribe_ids_ex([x], SR_IN, FC.BEAM, no_speech=False)[0].ids == good.ids
    finally:
        bare.close()
    # a callback that returns NaN, or a value that is no ratio: the call fails, the handle answers afterwards
    for value in (float("nan"), 0.0, -1.0):
        policy(nat, Script([value]))
        with pytest.raises(ValueError):
            nat.transcribe_ids_ex([x], SR_IN, FC.BEAM)
        assert nat.fallback_report() == []                           # (a failed call leaves no report)
        nat.set_fallback(None)
        assert nat.transcribe_ids_ex([x], SR_IN, FC.BEAM) == [good]
    # the report with too little room: the count, RT_ERR_LENGTH, nothing past the cap
    policy(nat, None)
    clips = ragged()
    n_win = sum(len(c.windows) for c in nat.transcribe_ids_ex(clips, SR_IN, FC.BEAM))
    att, n = (C.c_int32 * 4)(*[-7] * 4), C.c_int32()
    assert nat.lib.rt_stt_fallback_report(nat.handle, 2, att, None, None, C.byref(n)) == _native.RT_ERR_LENGTH and n.value == n_win > 4
    assert list(att) == [1, 1, -7, -7] and len(nat.fallback_report()) == n_win
    nat.set_fallback(None)
    assert nat.transcribe_ids_ex([x], SR_IN, FC.BEAM) == [good]


def test_whisper_tiny_dimensions(ctx):
    """51865 ids, one 30-s window, the first attempt failed by the script, best_of 5 at temperature 0.4, held to the restated loop.  The
    reference decides the case by the margins tests/stt_sample_cases.py records (TINY_CASE; tests/test_stt_fallback_cpu.py asserts
    them), so the comparison is unconditional."""
    cfg, state, x, want = FC.tiny_reference()
    assert F.decisive(want, FC.E, FC.G, FC.MARGIN)
    nat = S.NativeSTT(ctx, cfg, {k: v.cuda() for k, v in state.items()})
    try:
        s = Script([9.0])
        nat.set_fallback(FC.TINY_CASE["temperatures"], FC.BEST_OF, logprob_threshold=None, seed=FC.SEED, ratio=s.cb)
        got, = nat.transcribe_ids_ex([x], SR_IN, 1, no_speech=False)
        line, = nat.fallback_report()
        assert (line.attempts, line.temperature, line.compression_ratio, s.calls) == (2, pytest.approx(0.4), 1.0, 2)
        print("ids", got.ids, "|logprob - reference|", abs(got.windows[0].logprob - want.result.score))
        assert got.ids == want.result.ids and abs(got.windows[0].logprob - want.result.score) <= 4 * FC.E
    finally:
        nat.close()


def test_the_transcriber_takes_temperatures(ctx):
    clips = [K.CLIPS["clip(1.3, 3)"](), SC.CLIPS["clip(4.1, 5)"]()]
    plain = S.WhisperTranscriber(ctx, synthetic=True, cfg=CFG, beam_size=5)          # the default (0.0,) sets no policy
    try:
        want = plain.batch_detailed(clips, SR_IN)
        assert not plain.fallback and all(d.attempts == [] and d.temperature == [] and d.compression_ratio == [] for d in want)
        assert plain.model.fallback_report() == []
    finally:
        plain.close()
    for ts in (False, True):
        t = S.WhisperTranscriber(ctx, synthetic=True, cfg=CFG, beam_size=5, temperatures=(0.0, 0.4), logprob_threshold=-1.0, timestamps=ts)
        try:
            got = t.batch_detailed(clips, SR_IN)
            n_win = [len(c.windows) for c in (t.model.transcribe_ids_seek(clips, SR_IN, 5) if ts else t.model.transcribe_ids_ex(clips, SR_IN, 5))]
            assert [len(d.attempts) for d in got] == n_win == [len(d.temperature) for d in got] == [len(d.compression_ratio) for d in got]
            assert all(a in (1, 2) for d in got for a in d.attempts) and any(a == 2 for d in got for a in d.attempts)
            assert all(r > 0 for d in got for r in d.compression_ratio) and t.batch(clips, SR_IN) == [d.text for d in got]
            if ts:
                segs = t.batch_segments(clips, SR_IN)
                assert all(g.attempts in (1, 2) and g.compression_ratio > 0 and g.temperature in (0.0, pytest.approx(0.4)) for c in segs for g in c)
        finally:
            t.close()
    with pytest.raises(ValueError):
        S.WhisperTranscriber(ctx, synthetic=True, cfg=CFG, temperatures=(0.4, 0.2))
