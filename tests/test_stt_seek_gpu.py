"""Timestamps and seek on the GPU (rt_stt_transcribe_seek) against the float64 restatement of the two rules (tests/stt_seek_ref.py)
on the cases of tests/stt_seek_cases.py, whose conditions and margins tests/test_stt_seek_cpu.py asserts: ids, segment boundaries,
offsets and advances exact, every window's cumulative log-probability within 4 E.  And: a clip in a batch is the clip alone; a
discarded tail is decoded again (the test that cannot pass without the feature); the silence rule; the older entry points on a
handle with timestamps configured; Whisper-tiny dimensions; the argument rules; the caps.

Measured on an MI355X (this file prints the figures): see MEASURED in tests/stt_seek_cases.py."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

from oracle import whisper as OW
from rho_tts_amd import _native
from rho_tts_amd import stt as S
from tests import stt_seek_cases as SC
from tests import stt_seek_ref as SR
from tests.test_oracle_whisper import clip

pytestmark = pytest.mark.gpu

SR_IN = SC.SR
TICK = int(0.02 * SR_IN)
CFG = SC.seek_test_config()
WHOLE = CFG.n_timestamps - 1


@pytest.fixture(scope="module")
def ctx():
    c = _native.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def sets(ctx):
    """{set: (native model, oracle model)} on the configuration with timestamps."""
    made = {}
    for name, make in SC.STATES.items():
        state = make(CFG)
        made[name] = (S.NativeSTT(ctx, CFG, {k: v.cuda() for k, v in state.items()}), OW.build(CFG, state))
    yield made
    for nat, _ in made.values():
        nat.close()


def report(c):
    """What a clip's result is compared by: ids, segments in ticks, windows (offset, ids decoded, advance)."""
    return (c.ids, [(g.start_tick, g.end_tick, g.ids) for g in c.segments], [(w.offset, w.n_ids, w.advance) for w in c.windows])


def ref_report(c):
    return (c.ids, [(a, b, t) for a, b, t in c.segments], [(w.offset, len(w.ids), w.advance) for w in c.windows])


@pytest.mark.parametrize("B", [1, 5])
def test_cases_against_the_reference(sets, B):
    worst = 0.0
    for st, cl, mi, per in SC.CASES:
        nat, model = sets[st]
        x = SC.CLIPS[cl]()
        got, = nat.transcribe_ids_seek([x], SR_IN, B, max_initial_timestamp_index=mi, no_speech=False)
        want = SR.clip_transcribe(model, CFG, x, SR_IN, B, mi)
        errs = [abs(g.logprob - w.logprob) for g, w in zip(got.windows, want.windows)]
        worst = max([worst] + errs)
        print(f"set {st} {cl} max_initial {mi} B={B}: rounds {len(got.windows)} margin {want.margin:.3g} same {report(got) == ref_report(want)} "
              f"max |window logprob - reference| {max(errs):.3g}")
        assert want.margin >= SC.MARGIN and len(want.windows) == per[B][0]
        assert report(got) == ref_report(want), (st, cl, mi, B)
        assert max(errs) <= 4 * SC.E, (st, cl, mi, B, errs)
        assert abs(got.score - want.score) <= 4 * SC.E
        for g in got.segments:                                # seconds are ticks of 0.02 s
            assert g.start == pytest.approx(g.start_tick * 0.02, abs=1e-6) and g.end == pytest.approx(g.end_tick * 0.02, abs=1e-6)
        assert all(np.isnan(w.no_speech_prob) for w in got.windows) and got.language == CFG.prefix[1] and got.language_prob == 1.0
    print("E measured", worst, "recorded", SC.E, "bound", 4 * SC.E)


def ragged():
    """Eight clips from 0.4 s to 7 s: they finish in different rounds, and at width 5 (six windows to a group) a round spans two groups."""
    return [clip(0.4, SR_IN, 1), SC.CLIPS["clip(5.0, 2)"](), clip(2.0, SR_IN, 4), SC.CLIPS["clip(6.3, 11)"](), np.zeros(int(0.7 * SR_IN), dtype=np.float32),
            SC.CLIPS["clip(7.0, 3)"](), clip(3.1, SR_IN, 6), SC.CLIPS["clip(4.1, 5)"]()]


@pytest.mark.parametrize("B", [1, 5])
def test_a_clip_in_a_batch_is_the_clip_alone(sets, B):
    """Bit for bit - the dataclasses compare ids, float32 scores, times, offsets and no-speech probabilities - also in reversed order
    and with a detected language."""
    nat = sets["B"][0]
    clips = ragged()
    for lang in (None, "auto"):
        both = nat.transcribe_ids_seek(clips, SR_IN, B, lang, max_initial_timestamp_index=25)
        alone = [nat.transcribe_ids_seek([x], SR_IN, B, lang, max_initial_timestamp_index=25)[0] for x in clips]
        assert both == alone
        assert nat.transcribe_ids_seek(clips[::-1], SR_IN, B, lang, max_initial_timestamp_index=25) == both[::-1]
        rounds = [len(c.windows) for c in both]
        assert len(set(rounds)) >= 3 and max(rounds) >= 4 and min(rounds) == 1, rounds
        assert all(np.isfinite(w.no_speech_prob) for c in both for w in c.windows)
    assert len(clips) > 32 // 5


def test_a_discarded_tail_is_decoded_again(sets):
    """The case of kind (a): the first window closes its last pair below a whole window and discards the ids behind it; the second
    window starts at that pair's tick, and the clip's ids are not those of fixed 2-s cuts (transcribe_ids_ex)."""
    st, cl, mi = SC.REDECODED
    nat, model = sets[st]
    x = SC.CLIPS[cl]()
    got, = nat.transcribe_ids_seek([x], SR_IN, 1, max_initial_timestamp_index=mi)
    first, second = got.windows[0], got.windows[1]
    pair_end = max(g.end_tick for g in got.segments if g.end_tick <= first.advance)
    assert 0 < first.advance < WHOLE and second.offset == first.advance * TICK == pair_end * TICK
    n_first = sum(len(g.ids) for g in got.segments if g.end_tick <= first.advance)
    assert first.n_ids > n_first + 3                          # (three timestamps at least, and a tail that is not in the clip's ids)
    fixed = nat.transcribe_ids_ex([x], SR_IN, 1)[0]
    assert got.ids != fixed.ids and got.ids and fixed.ids
    assert len(fixed.windows) == 3 and [w.offset for w in got.windows] != [k * WHOLE * TICK for k in range(len(got.windows))]


def test_the_silence_rule(sets):
    o = SC.SILENCE
    nat, model = sets[o["set"]]
    x = SC.speech_then_silence()
    kw = dict(max_initial_timestamp_index=o["max_initial"])
    got, = nat.transcribe_ids_seek([x], SR_IN, 1, no_speech_threshold=o["no_speech_threshold"], logprob_threshold=o["logprob_threshold"], **kw)
    speech, = nat.transcribe_ids_seek([x[:2 * SR_IN]], SR_IN, 1, **kw)
    want = SR.clip_transcribe(model, CFG, x, SR_IN, 1, o["max_initial"], None, o["no_speech_threshold"], o["logprob_threshold"])
    print([(w.offset, w.advance, w.no_speech_prob, w.avg_logprob) for w in got.windows])
    assert [(w.offset, w.advance) for w in got.windows] == [(0, WHOLE), (WHOLE * TICK, WHOLE), (2 * WHOLE * TICK, WHOLE)]
    assert all(g.end_tick <= WHOLE for g in got.segments) and got.segments == speech.segments and got.ids == speech.ids and got.ids
    assert report(got) == ref_report(want)
    for g, w in zip(got.windows, want.windows):
        assert abs(np.log(g.no_speech_prob) - np.log(w.no_speech_prob)) <= 4 * SC.E and abs(g.logprob - w.logprob) <= 4 * SC.E
    assert got.score == speech.score                          # (the kept windows' alone)
    # without thresholds the windows of zeros are transcribed like any other
    loud, = nat.transcribe_ids_seek([x], SR_IN, 1, **kw)
    assert len(loud.segments) > len(got.segments)


def test_existing_paths_are_what_they_are_without_timestamps(ctx, sets):
    """transcribe_ids_ex and transcribe_ids_beam on a handle with timestamps configured return the bits of a handle without."""
    plain_cfg = dataclasses.replace(CFG, timestamp_begin=None)
    plain = S.NativeSTT(ctx, plain_cfg, {k: v.cuda() for k, v in SC.state_b(CFG).items()})
    try:
        nat = sets["B"][0]
        clips = ragged()
        for B in (1, 5):
            assert nat.transcribe_ids_beam(clips, SR_IN, B) == plain.transcribe_ids_beam(clips, SR_IN, B)
            for lang in (None, "auto"):
                assert nat.transcribe_ids_ex(clips, SR_IN, B, lang) == plain.transcribe_ids_ex(clips, SR_IN, B, lang)
        nat.transcribe_ids_seek(clips[:2], SR_IN, 5)          # ... also after the seek path has used the shared buffers
        assert nat.transcribe_ids_ex(clips, SR_IN, 5, "auto") == plain.transcribe_ids_ex(clips, SR_IN, 5, "auto")
        assert nat.transcribe_ids_batch(clips, SR_IN) == plain.transcribe_ids_batch(clips, SR_IN)
        with pytest.raises(ValueError):                       # no timestamps configured: refused, and the handle stays usable
            plain.transcribe_ids_seek(clips[:1], SR_IN)
        xs, n, ptrs, lens = plain._clips(clips[:1])
        opts, out = S.RtSttSeekOpts(), S.RtSttSeekOut()
        opts.beam_size, opts.max_tokens, opts.max_initial_timestamp_index = 1, 12, -1
        toks, cnt = (C.c_int32 * 12)(), (C.c_int32 * 1)()
        out.h_tokens, out.h_n_tokens, out.segment_cap, out.window_cap = toks, cnt, 4, 4
        assert plain.lib.rt_stt_transcribe_seek(plain.handle, ptrs, lens, 1, SR_IN, C.byref(opts), C.byref(out)) == _native.RT_ERR_INVALID
        assert plain.transcribe_ids_batch(clips[:1], SR_IN) == nat.transcribe_ids_batch(clips[:1], SR_IN)
    finally:
        plain.close()


def test_timestamps_on_a_handle_without_languages(ctx, sets):
    """A handle with timestamp ids and no language ids: the seek path without a probe and the plain beam call return the bits of the
    handle with languages; detection and the silence rule are refused, and the handle answers afterwards."""
    bare = S.NativeSTT(ctx, dataclasses.replace(CFG, languages={}), {k: v.cuda() for k, v in SC.state_b(CFG).items()})

    def no_probe(c):
        """The clip with its windows' no-speech probabilities - all NaN, which never compares equal - set aside."""
        assert c.windows and all(np.isnan(w.no_speech_prob) for w in c.windows)
        return dataclasses.replace(c, windows=[dataclasses.replace(w, no_speech_prob=0.0) for w in c.windows])
    try:
        nat = sets["B"][0]
        clips = ragged()[:3]
        kw = dict(max_initial_timestamp_index=25, no_speech=False)
        for B in (1, 5):
            got, want = bare.transcribe_ids_seek(clips, SR_IN, B, **kw), nat.transcribe_ids_seek(clips, SR_IN, B, **kw)
            assert [no_probe(c) for c in got] == [no_probe(c) for c in want]
            assert all(c.language == CFG.prefix[1] and c.language_prob == 1.0 for c in got)
            with pytest.raises(ValueError):
                bare.transcribe_ids_seek(clips, SR_IN, B, "auto", **kw)
            with pytest.raises(ValueError):
                bare.transcribe_ids_seek(clips, SR_IN, B, no_speech_threshold=0.6, **kw)
            assert [no_probe(c) for c in bare.transcribe_ids_seek(clips, SR_IN, B, **kw)] == [no_probe(c) for c in got]
            assert bare.transcribe_ids_beam(clips, SR_IN, B) == nat.transcribe_ids_beam(clips, SR_IN, B)
    finally:
        bare.close()


def test_whisper_tiny_dimensions(ctx):
    """51865 ids of which 1501 are timestamps, 30-s windows: a 31-s clip (two rounds) and a 4-s clip at width 1.  A clip is held to
    the reference - ids, segments, offsets, every window's score within 4 E - where the reference's margin meets the constant; on the
    CPU both clips' do (3.4e-2 and 1.0e-2), and at most one may fall below it here."""
    cfg = S.SttConfig(max_new_tokens=8, timestamp_begin=50364)
    state = S.synthetic_state(cfg, 789)
    nat = S.NativeSTT(ctx, cfg, {k: v.cuda() for k, v in state.items()})
    try:
        clips = [clip(31.0, SR_IN, 7), clip(4.0, SR_IN, 3)]
        got = nat.transcribe_ids_seek(clips, SR_IN, 1)        # (with the probe pass: a NaN no-speech probability would not compare equal)
        assert got == [nat.transcribe_ids_seek([x], SR_IN, 1)[0] for x in clips]
        model = OW.build(cfg, state)
        held, worst = 0, 0.0
        for x, g in zip(clips, got):
            want = SR.clip_transcribe(model, cfg, x, SR_IN, 1, cfg.max_initial_timestamp_index)
            same = report(g) == ref_report(want)
            errs = [abs(a.logprob - b.logprob) for a, b in zip(g.windows, want.windows)] if same else []
            worst = max([worst] + errs)
            print(f"{len(x) / SR_IN:.0f} s: rounds {len(g.windows)} margin {want.margin:.3g} same {same} max |window logprob - reference| {max(errs or [float('nan')]):.3g}")
            if want.margin < SC.MARGIN:
                continue                                      # (the reference itself does not decide this clip by the margin)
            held += 1
            assert same and max(errs) <= 4 * SC.E
        print("E measured at Whisper-tiny dimensions", worst)
        assert held >= 1 and len(got[0].windows) >= 2 and len(got[1].windows) == 1
    finally:
        nat.close()


def test_arguments_and_caps(sets):
    nat = sets["A"][0]
    x = SC.CLIPS["clip(5.0, 2)"]()
    full, = nat.transcribe_ids_seek([x], SR_IN, 1, max_initial_timestamp_index=25)
    assert len(full.windows) > 1 and len(full.segments) > 1
    # caps of one: the wrapper repeats the call once with the reported counts and returns the full result
    assert nat.transcribe_ids_seek([x], SR_IN, 1, max_initial_timestamp_index=25, caps=(1, 1, 1)) == [full]
    xs, n, ptrs, lens = nat._clips([x])

    def call(beam=1, seg_cap=8, win_cap=8, max_tokens=12):
        opts, out = S.RtSttSeekOpts(), S.RtSttSeekOut()
        opts.beam_size, opts.max_tokens, opts.max_initial_timestamp_index = beam, max_tokens, 25
        opts.no_speech_threshold = opts.logprob_threshold = float("nan")
        toks, cnt = (C.c_int32 * max(max_tokens, 1))(), (C.c_int32 * 1)()
        seg, win = (C.c_int32 * 8)(*[-7] * 8), (C.c_int32 * 8)(*[-7] * 8)
        out.h_tokens, out.h_n_tokens, out.h_seg_n_ids, out.h_win_n_ids, out.segment_cap, out.window_cap = toks, cnt, seg, win, seg_cap, win_cap
        return nat.lib.rt_stt_transcribe_seek(nat.handle, ptrs, lens, 1, SR_IN, C.byref(opts), C.byref(out)), out, list(seg), list(win)
    for bad in (dict(beam=0), dict(beam=9), dict(seg_cap=0), dict(win_cap=0), dict(max_tokens=0)):
        assert call(**bad)[0] == _native.RT_ERR_INVALID, bad
    rc, out, seg, win = call(seg_cap=1, win_cap=2)            # nothing past a cap, and the counts a repeat needs
    assert rc == _native.RT_ERR_LENGTH and (out.n_segments, out.n_windows) == (len(full.segments), len(full.windows))
    assert seg[1:] == [-7] * 7 and win[2:] == [-7] * 6 and seg[0] == len(full.segments[0].ids) and win[:2] == [w.n_ids for w in full.windows[:2]]
    rc, out, seg, win = call()
    assert rc == _native.RT_OK and out.max_clip_tokens == len(full.ids)
    with pytest.raises(ValueError):
        nat.transcribe_ids_seek([x], 10)
    assert nat.transcribe_ids_seek([], SR_IN) == []
    assert nat.transcribe_ids_seek([x], SR_IN, 1, max_initial_timestamp_index=25) == [full]      # the handle stays usable


def test_the_transcriber_takes_timestamps(ctx):
    with pytest.raises(ValueError):                           # a configuration without timestamp ids raises at construction
        S.WhisperTranscriber(ctx, synthetic=True, cfg=S.tiny_test_config(), timestamps=True)
    t = S.WhisperTranscriber(ctx, synthetic=True, cfg=dataclasses.replace(CFG, max_initial_timestamp_index=25), timestamps=True, beam_size=5)
    try:
        clips = [SC.CLIPS["clip(5.0, 2)"](), clip(0.4, SR_IN, 1)]
        want = t.model.transcribe_ids_seek(clips, SR_IN, 5)
        texts = t.batch(clips, SR_IN)
        assert texts == [S.join_segment_texts(" ".join(f"<{i}>" for i in g.ids) for g in c.segments) for c in want]
        assert t.ids_batch(clips, SR_IN) == [c.ids for c in want] and t(clips[0], SR_IN) == texts[0] and t.ids(clips[0], SR_IN) == want[0].ids
        assert t.batch_scored(clips, SR_IN) == [(x, c.score) for x, c in zip(texts, want)]
        segs = t.batch_segments(clips, SR_IN)
        assert [[(g.start, g.end, g.ids) for g in c] for c in segs] == [[(g.start, g.end, g.ids) for g in c.segments] for c in want]
    finally:
        t.close()
