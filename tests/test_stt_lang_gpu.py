"""Per-clip language, detection and no-speech end to end (rt_stt_set_languages, rt_stt_detect_language, rt_stt_transcribe_ex)
on the smallest model with a language slot (tests/stt_lang_cases.py) under weight sets A and B of the beam tests, against the float64
restatement (tests/stt_lang_ref.py) on transformers' Whisper, and at Whisper-tiny dimensions.

Bounds: the detected id is exact (every case's language margin is at least K.MARGIN: tests/test_stt_lang_cpu.py); the language and
no-speech log-probabilities agree with the oracle within 4 E, E = 3e-5 being the project's recorded device-to-oracle
log-probability error (tests/stt_beam_cases.py).  Measured on an MI355X: see MEASURED in tests/stt_lang_cases.py."""
import ctypes as C
import dataclasses
import math

import numpy as np
import pytest
import torch

from oracle import whisper as OW
from rho_tts_amd import _native
from rho_tts_amd import stt as S
from tests import stt_beam_ref as R
from tests import stt_lang_cases as L
from tests import stt_lang_ref as LR
from tests.test_oracle_whisper import clip
from tests.test_stt_batch_gpu import ragged_clips

pytestmark = pytest.mark.gpu

SR = L.SR


@pytest.fixture(scope="module")
def ctx():
    c = _native.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def tiny(ctx):
    """(cfg, {set: (native model, oracle model)}, first-window log-mels of the ragged clips)."""
    cfg = L.lang_test_config()
    sets = {}
    for name, make in L.STATES.items():
        state = make(cfg)
        sets[name] = (S.NativeSTT(ctx, cfg, {k: v.cuda() for k, v in state.items()}), OW.build(cfg, state))
    yield cfg, sets, LR.first_window_mels(cfg, ragged_clips(), SR)
    for nat, _ in sets.values():
        nat.close()


def dlog(p, want_log):
    return abs(math.log(p) - want_log)


def same(a, b):
    """Two reports of transcribe_ids_ex, bit for bit (a NaN no-speech probability - no probe - equals itself)."""
    def key(c):
        return (c.ids, c.score, c.language, c.language_prob, [(w.n_ids, w.logprob, repr(w.no_speech_prob)) for w in c.windows])
    return [key(c) for c in a] == [key(c) for c in b]


def test_detection_against_the_oracle(tiny):
    cfg, sets, mels = tiny
    clips = ragged_clips()
    worst_l = worst_n = 0.0
    langs = set()
    for name, (nat, model) in sets.items():
        got = nat.detect_language(clips, SR)
        ex = nat.transcribe_ids_ex(clips, SR, 1, "auto")
        for i, (mel, (lang, prob, ns)) in enumerate(zip(mels, got)):
            want = LR.detect(model, cfg, mel)
            el, en = dlog(prob, want.log_language_prob), dlog(ns, want.log_no_speech_prob)
            print(f"set {name} clip {i}: language {lang} (oracle {want.language}, margin {want.margin:.3g}) p {prob:.4f} |dlog| {el:.3g}; "
                  f"no-speech {ns:.3g} |dlog| {en:.3g}")
            worst_l, worst_n = max(worst_l, el), max(worst_n, en)
            assert want.margin >= L.MARGIN and lang == want.language, (name, i)
            # the transcribing call decides alike, from the same three numbers
            assert (ex[i].language, ex[i].language_prob, ex[i].windows[0].no_speech_prob) == (lang, prob, ns)
            langs.add(lang)
    print(f"max |dlog p| language {worst_l:.3g} no-speech {worst_n:.3g}; bound 4 E = {4 * L.E:.3g}; recorded {L.MEASURED}")
    assert worst_l <= 4 * L.E and worst_n <= 4 * L.E
    assert len(langs) >= 2


@pytest.mark.parametrize("B", [1, 5])
def test_forced_equals_detected(tiny, B):
    cfg, sets, _ = tiny
    clips = ragged_clips()
    for name, (nat, _) in sets.items():
        auto = nat.transcribe_ids_ex(clips, SR, B, "auto")
        forced = nat.transcribe_ids_ex(clips, SR, B, [c.language for c in auto])
        assert [(c.ids, c.score, c.language) for c in auto] == [(c.ids, c.score, c.language) for c in forced] and any(c.ids for c in auto)
        assert [[(w.n_ids, w.logprob, w.no_speech_prob) for w in c.windows] for c in auto] == [[(w.n_ids, w.logprob, w.no_speech_prob) for w in c.windows] for c in forced]
        assert all(c.language_prob == 1.0 for c in forced) and all(0.25 < c.language_prob < 1.0 for c in auto)
        assert len({c.language for c in auto}) >= 2
        # the configuration's own language: the existing entry, by every route
        ids, scores = nat.transcribe_ids_beam(clips, SR, B)
        for how in ("en", None):
            for no_speech in (True, False):
                own = nat.transcribe_ids_ex(clips, SR, B, how, no_speech=no_speech)
                assert [c.ids for c in own] == ids and [c.score for c in own] == scores, (name, how, no_speech)
                assert all(c.language == cfg.languages["en"] and c.language_prob == 1.0 for c in own)
        # a window's report adds up to the clip's
        for c in auto:
            assert sum(w.n_ids for w in c.windows) == len(c.ids)
            total = sum(w.logprob for w in c.windows) / sum(w.n_ids + 1 for w in c.windows)
            assert abs(c.score - total) <= 1e-6 * max(1.0, abs(total))


def test_a_clip_in_a_batch_is_the_clip_alone(tiny):
    """Ten windows at width 5: a group holds six, so the call runs two groups and the three-window 5.3-s clip straddles them - its
    third window takes the language its first window was given in the group before."""
    cfg, sets, _ = tiny
    clips = ragged_clips()
    nat = sets["A"][0]
    assert [nat.windows(len(x), SR) for x in clips] == [1, 1, 2, 1, 1, 3, 1]
    got = nat.transcribe_ids_ex(clips, SR, 5, "auto")
    alone = [nat.transcribe_ids_ex([x], SR, 5, "auto")[0] for x in clips]
    assert same(got, alone)
    assert same(nat.transcribe_ids_ex(clips[::-1], SR, 5, "auto"), got[::-1])
    det = nat.detect_language(clips, SR)
    assert [(c.language, c.language_prob) for c in got] == [(d[0], d[1]) for d in det] and det == [nat.detect_language([x], SR)[0] for x in clips]
    # every window of the long clip carries its first window's language: forced to it, window by window, the windows are the clip's
    long, lang = clips[5], got[5].language
    win = cfg.chunk_seconds * SR
    parts = [nat.transcribe_ids_ex([long[k * win:(k + 1) * win]], SR, 5, lang)[0] for k in range(3)]
    assert got[5].ids == sum((p.ids for p in parts), [])
    assert [(w.n_ids, w.logprob, w.no_speech_prob) for w in got[5].windows] == [(p.windows[0].n_ids, p.windows[0].logprob, p.windows[0].no_speech_prob) for p in parts]
    # ... and not what its later windows would be given on their own, where that differs
    later = [nat.detect_language([long[k * win:(k + 1) * win]], SR)[0][0] for k in (1, 2)]
    print("5.3-s clip: first window", lang, "later windows on their own", later)
    # a clip whose later windows would be given ANOTHER language on their own (speech, then silence), straddling the two groups:
    # windows 5, 6, 7 of the call.  Its silent windows are decoded under the first window's language all the same.
    turn = np.concatenate([clips[4], np.zeros(int(3.3 * SR), dtype=np.float32)])
    batch = clips[:4] + [turn]
    assert sum(nat.windows(len(x), SR) for x in batch[:4]) == 5 and nat.windows(len(turn), SR) == 3
    t_got = nat.transcribe_ids_ex(batch, SR, 5, "auto")[4]
    own = [nat.detect_language([turn[k * win:(k + 1) * win]], SR)[0][0] for k in range(3)]
    print("speech-then-silence clip: windows on their own", own, "the clip", t_got.language)
    assert t_got.language == own[0] and own[1] != own[0] and own[2] != own[0]
    carried = [nat.transcribe_ids_ex([turn[k * win:(k + 1) * win]], SR, 5, own[0])[0] for k in range(3)]
    apart = [nat.transcribe_ids_ex([turn[k * win:(k + 1) * win]], SR, 5, own[k])[0] for k in range(3)]
    rep = lambda cs: [(c.windows[0].n_ids, c.windows[0].logprob) for c in cs]                                  # noqa: E731
    assert [(w.n_ids, w.logprob) for w in t_got.windows] == rep(carried) != rep(apart)
    assert t_got.ids == sum((c.ids for c in carried), []) and same([t_got], nat.transcribe_ids_ex([turn], SR, 5, "auto"))
    # mixed requests in one call: each clip as it is alone
    req = ["auto", "zh", "auto", "ko", "en", "ja", "auto"]
    mixed = nat.transcribe_ids_ex(clips, SR, 5, req)
    assert same(mixed, [nat.transcribe_ids_ex([x], SR, 5, [r])[0] for x, r in zip(clips, req)])
    assert [c.language for c in mixed][1::2] == [cfg.languages[k] for k in ("zh", "ko", "ja")]


def test_different_languages(ctx, tiny):
    """A clip forced to two languages: each is what a handle CONFIGURED with that language gives (ids and scores bit for bit), whose
    logits behind the prefix are the oracle's with that prefix; the two differ; and the ids are the oracle's under the margin rule."""
    cfg, sets, mels = tiny
    state = L.STATES["B"](cfg)
    nat, model = sets["B"]
    x, mel = ragged_clips()[0], mels[0]
    firsts = {}
    for code in ("en", "ko"):
        c2 = cfg.with_language(code)
        other = S.NativeSTT(ctx, c2, {k: v.cuda() for k, v in state.items()})
        try:
            ids_cfg, first = other.transcribe_ids(x, SR, first_logits=True)
            beam_cfg = other.transcribe_ids_beam([x], SR, 1)
        finally:
            other.close()
        got = nat.transcribe_ids_ex([x], SR, 1, code)[0]
        assert (got.ids, got.score) == (beam_cfg[0][0], beam_cfg[1][0]) and got.ids == ids_cfg and got.language == cfg.languages[code]
        ids_o, first_o = OW.greedy(model, c2, mel)
        err = float((first.cpu() - first_o).abs().max()) / float(first_o.std())
        want = R.beam_search(model, c2, mel, 1)
        print(f"{code}: logits behind the prefix |device - oracle| {err:.3g} sigma, margin {want.margin:.3g}, ids same {got.ids == want.ids}")
        assert err < 2e-3 and want.ids == ids_o
        if want.margin >= L.MARGIN:
            assert got.ids == want.ids
        firsts[code] = (first.cpu(), first_o)
    dev_gap = float((firsts["en"][0] - firsts["ko"][0]).abs().max()) / float(firsts["en"][1].std())
    assert dev_gap > 0.05                                    # (the device error is held to 2e-3 sigma above)


def test_the_silence_rule_end_to_end(ctx):
    """A threshold just below the oracle's no-speech probability of one clip: that clip is "", one window dropped; the others and
    the default (no threshold) are today's texts."""
    cfg = L.lang_test_config()
    model = OW.build(cfg, S.synthetic_state(cfg, 789))
    clips = ragged_clips()[:2] + ragged_clips()[3:5]        # one window each (the empty clip would tie with the silent one)
    ns = [math.exp(LR.detect(model, cfg, m).log_no_speech_prob) for m in LR.first_window_mels(cfg, clips, SR)]
    order = np.argsort(ns)
    top, second = int(order[-1]), int(order[-2])
    t = math.sqrt(ns[top] * ns[second])
    print("oracle no-speech probabilities", ns, "threshold", t)
    assert math.log(ns[top] / t) > 100 * L.E and math.log(t / ns[second]) > 100 * L.E
    plain = S.WhisperTranscriber(ctx, synthetic=True, cfg=cfg)
    ruled = S.WhisperTranscriber(ctx, synthetic=True, cfg=cfg, no_speech_threshold=t, logprob_threshold=0.0)
    try:
        today = plain.batch(clips, SR)
        assert today == [plain(x, SR) for x in clips] and all(today)
        texts = ruled.batch(clips, SR)
        assert texts == [("" if i == top else today[i]) for i in range(len(clips))]
        assert ruled(clips[top], SR) == "" and ruled(clips[second], SR) == today[second]
        det = ruled.batch_detailed(clips, SR)
        assert [d.windows_dropped for d in det] == [1 if i == top else 0 for i in range(len(clips))]
        assert det[top].ids == [] and det[top].text == "" and all(d.language == "en" and d.language_prob == 1.0 for d in det)
        assert all(abs(math.log(d.no_speech_prob / p)) <= 4 * L.E for d, p in zip(det, ns))
        assert [d.text for d in plain.batch_detailed(clips, SR)] == today and all(d.windows_dropped == 0 for d in plain.batch_detailed(clips, SR))
    finally:
        plain.close()
        ruled.close()


def test_whisper_tiny_dimensions(ctx):
    """head_dim 64 x 6 heads, 1500 encoder positions, 99 languages in a vocabulary of 51865: alone equals batched, the probabilities
    are the oracle's, and so is the language wherever its margin meets the constant."""
    cfg = S.SttConfig(max_new_tokens=8)
    assert len(cfg.languages) == 99
    state = S.synthetic_state(cfg, 789)
    nat = S.NativeSTT(ctx, cfg, {k: v.cuda() for k, v in state.items()})
    try:
        clips = [clip(0.8, SR, 0), clip(3.3, SR, 3), clip(9.0, SR, 7)]
        got = nat.transcribe_ids_ex(clips, SR, 5, "auto")
        assert same(got, [nat.transcribe_ids_ex([x], SR, 5, "auto")[0] for x in clips]) and all(c.ids for c in got)
        det = nat.detect_language(clips, SR)
        assert [(c.language, c.language_prob, c.windows[0].no_speech_prob) for c in got] == det
        model = OW.build(cfg, state)
        held, worst_l, worst_n = 0, 0.0, 0.0
        for x, (lang, prob, ns) in zip(clips, det):
            want = LR.detect(model, cfg, R.window_mels(cfg, x, SR)[0])
            el, en = dlog(prob, want.log_language_prob), dlog(ns, want.log_no_speech_prob)
            print(f"language {lang} (oracle {want.language}, margin {want.margin:.3g}) p {prob:.4g} |dlog| {el:.3g}; no-speech {ns:.3g} |dlog| {en:.3g}")
            worst_l, worst_n = max(worst_l, el), max(worst_n, en)
            if want.margin >= L.MARGIN:
                held += 1
                assert lang == want.language
        print(f"max |dlog p| language {worst_l:.3g} no-speech {worst_n:.3g}; bound 4 E = {4 * L.E:.3g}")
        assert worst_l <= 4 * L.E and worst_n <= 4 * L.E and held >= 1
    finally:
        nat.close()


def ex_call(nat, x, languages, beam=2, window_cap=8, max_tokens=12, no_speech=True):
    """rt_stt_transcribe_ex on one clip by hand: (status, n_windows)."""
    xs = nat._pcm(x)
    ptrs, lens = (C.c_void_p * 1)(xs.data_ptr()), (C.c_int64 * 1)(xs.numel())
    opts, out = S.RtSttDecodeOpts(), S.RtSttDecodeOut()
    opts.beam_size, opts.max_tokens = beam, max_tokens
    keep = [(C.c_int32 * max_tokens)(), (C.c_int32 * 1)(), (C.c_int32 * 8)(), (C.c_float * 8)()]
    if languages is not None:
        keep.append((C.c_int32 * 1)(languages))
        opts.h_language = keep[-1]
    out.h_tokens, out.h_n_tokens, out.h_win_clip, out.window_cap = keep[0], keep[1], keep[2], window_cap
    if no_speech:
        out.h_win_no_speech = keep[3]
    return nat.lib.rt_stt_transcribe_ex(nat.handle, ptrs, lens, 1, SR, C.byref(opts), C.byref(out)), out.n_windows


def test_arguments(ctx, tiny):
    cfg, sets, _ = tiny
    nat = sets["A"][0]
    INVALID = _native.RT_ERR_INVALID
    x = clip(0.4, SR, 1)
    long = clip(5.3, SR, 11)
    good = nat.transcribe_ids_ex([x, long], SR, 2, "auto")
    assert ex_call(nat, x, -1) == (0, 1) and ex_call(nat, long, -1) == (0, 3)
    for bad in (7, 291, 296, 299, 300, -2, 1 << 30):                      # neither -1 nor a configured id
        assert ex_call(nat, x, bad)[0] == INVALID
    assert ex_call(nat, long, -1, window_cap=2)[0] == INVALID             # three windows, room for two
    assert ex_call(nat, long, -1, window_cap=3) == (0, 3)
    assert ex_call(nat, x, -1, beam=0)[0] == INVALID and ex_call(nat, x, -1, beam=9)[0] == INVALID
    assert nat.transcribe_ids_ex([], SR, 2, "auto") == [] and nat.detect_language([], SR) == []
    with pytest.raises(ValueError):
        nat.transcribe_ids_ex([x], SR, 2, "de")
    with pytest.raises(ValueError):
        nat.transcribe_ids_ex([x], SR, 2, ["en", "zh"])
    assert same(nat.transcribe_ids_ex([x, long], SR, 2, "auto"), good)    # the handle is usable, and gives what it gave
    # a handle without languages: every request for one, and for no-speech probabilities, is refused; the plain call works
    plain_cfg = S.tiny_test_config()
    plain = S.NativeSTT(ctx, plain_cfg, {k: v.cuda() for k, v in S.synthetic_state(plain_cfg, 789).items()})
    try:
        assert ex_call(plain, x, -1)[0] == INVALID and ex_call(plain, x, 292)[0] == INVALID and ex_call(plain, x, None)[0] == INVALID
        assert ex_call(plain, x, None, no_speech=False) == (0, 1)
        lang = (C.c_int32 * 1)()
        xs = plain._pcm(x)
        assert plain.lib.rt_stt_detect_language(plain.handle, (C.c_void_p * 1)(xs.data_ptr()), (C.c_int64 * 1)(xs.numel()), 1, SR, lang, None, None) == INVALID
        own = plain.transcribe_ids_ex([x], SR, 2, None, no_speech=False)[0]
        assert (([own.ids], [own.score]) == plain.transcribe_ids_beam([x], SR, 2)) and math.isnan(own.windows[0].no_speech_prob)
    finally:
        plain.close()
    # rt_stt_set_languages: a prefix without a language slot, prefix[1] not in the list, ids outside the vocabulary, after finalize
    ids = (C.c_int32 * 4)(292, 293, 294, 295)
    assert nat.lib.rt_stt_set_languages(nat.handle, ids, 4, 297) == _native.RT_ERR_STATE
    for c2, lang_ids, ns in ((dataclasses.replace(plain_cfg, prefix=(291,)), [292, 293], 297), (cfg, [293, 294], 297), (cfg, [292, 300], 297),
                             (cfg, [292, -1], 297), (cfg, [292, 293], 300), (cfg, [], 297), (cfg, [292] * 129, 297)):
        h = C.c_void_p()
        rc = S._rt_config(c2)
        ctx.check(nat.lib.rt_stt_create(ctx.handle, C.byref(rc), C.byref(h)), "rt_stt_create")
        try:
            arr = (C.c_int32 * max(len(lang_ids), 1))(*lang_ids)
            assert nat.lib.rt_stt_set_languages(h, arr, len(lang_ids), ns) == INVALID, (c2.prefix, lang_ids, ns)
            assert nat.lib.rt_stt_set_languages(h, ids, 4, 297) == (INVALID if len(c2.prefix) < 2 else 0)
        finally:
            nat.lib.rt_stt_destroy(h)
    with pytest.raises(Exception):
        S.NativeSTT(ctx, dataclasses.replace(cfg, prefix=(291, 296, 296, 298)), {k: v.cuda() for k, v in S.synthetic_state(cfg, 789).items()})


def test_provider_validates_a_chinese_voice_with_the_chinese_prefix(monkeypatch):
    """A voice that speaks Chinese is transcribed as Chinese: the provider's language name picks the transcriber's language, a chunk
    is validated through ``transcriber.batch`` in one native call, and the prefix the native side used - read back through
    ``batch_detailed`` - carries the zh id."""
    from rho_tts_amd.provider import MI355XQwenTTS
    cfg = L.lang_test_config()
    texts = ["A short sentence to validate.", "And another one.", "The third text."]
    t = MI355XQwenTTS(device="cuda", speaker="Vivian", model_path="x/CustomVoice-small", batch_size=4, max_iterations=2, language="Chinese")
    try:
        eng = t._load_engine()
        assert S.whisper_language(t.language) == "zh"
        tr = S.WhisperTranscriber(eng.ctx, synthetic=True, cfg=cfg, language=S.whisper_language(t.language))
        assert tr.cfg.prefix == (291, cfg.languages["zh"], 296, 298) and cfg.prefix[1] == cfg.languages["en"]
        calls, seen = [], []
        batch = tr.batch

        def counted(audios, sr):
            calls.append(len(audios))
            seen.extend(tr.batch_detailed(audios, sr))
            return batch(audios, sr)
        monkeypatch.setattr(tr, "batch", counted)
        t.transcriber = tr
        t.drift_scorer = lambda audio, sr: 0.01
        t.drift_scorer.batch = lambda audios, sr: [0.01] * len(audios)
        t.text_similarity_threshold = 0.0
        res = t.generate(texts)
        assert res is not None and all(r is not None and r.text_similarity is not None for r in res)
        assert calls and sum(calls) >= len(texts)
        assert seen and all(d.language == "zh" and d.language_prob == 1.0 for d in seen)
        # the same audio under the English prefix reads differently: the prefix is in force
        en = S.WhisperTranscriber(eng.ctx, synthetic=True, cfg=cfg)
        try:
            x = clip(1.3, SR, 3)
            assert en.batch_detailed([x], SR)[0].language == "en"
            assert tr.model.transcribe_ids_ex([x], SR, 1, "en")[0].ids == en.ids(x, SR)
            assert tr.ids(x, SR) == en.model.transcribe_ids_ex([x], SR, 1, "zh")[0].ids
        finally:
            en.close()
        tr.close()
    finally:
        t.close()
