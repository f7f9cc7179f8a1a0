"""Timestamps and seek on the CPU: the fixtures' conditions and margins (tests/stt_seek_cases.py), the float64 restatement of the two
rules (tests/stt_seek_ref.py) against transformers' own WhisperTimeStampLogitsProcessor and _retrieve_segment, the restated loop
against transformers' long-form generate, and the Python wrapper's logic (cap sizing and the one repeat, the join of segment texts,
the construction errors) on a stand-in for the library."""
import ctypes as C
import dataclasses
import types

import numpy as np
import pytest
import torch

from oracle import whisper as OW
from rho_tts_amd import _native
from rho_tts_amd import stt as S
from tests import stt_seek_cases as SC
from tests import stt_seek_ref as SR

CFG = SC.seek_test_config()
T0, EOS, V = CFG.timestamp_begin, CFG.eos_id, CFG.vocab
WHOLE = CFG.n_timestamps - 1


@pytest.fixture(scope="module")
def models():
    return {k: OW.build(CFG, make(CFG)) for k, make in SC.STATES.items()}


@pytest.fixture(scope="module")
def solved(models):
    """Every case at widths 1 and 5 on the reference, computed once."""
    return {(st, cl, mi, B): SR.clip_transcribe(models[st], CFG, SC.CLIPS[cl](), SC.SR, B, mi) for st, cl, mi, per in SC.CASES for B in per}


# ---------------------------------------------------------------------------------------------- (i) the fixtures
def test_the_configuration_holds_the_timestamps():
    assert (V, T0, CFG.n_timestamps, CFG.prefix) == (400, 299, 101, (291, 292, 296, 298)) and T0 + CFG.n_timestamps == V
    S.check_timestamp_config(CFG, True)


def test_every_case_has_its_recorded_rounds_and_margin(solved):
    for (st, cl, mi, B), c in solved.items():
        rounds, margin = next(per[B] for s_, c_, m_, per in SC.CASES if (s_, c_, m_) == (st, cl, mi))
        print(st, cl, mi, B, len(c.windows), f"{c.margin:.3g}")
        assert len(c.windows) == rounds and 3 <= rounds <= 6, (st, cl, mi, B, len(c.windows))
        assert c.margin >= SC.MARGIN, (st, cl, mi, B, c.margin)
        assert c.margin == pytest.approx(margin, rel=0.05), (st, cl, mi, B, c.margin)


def _shape(w):
    ts = [t >= T0 for t in w.ids]
    pairs = [k for k in range(len(ts) - 1) if ts[k] and ts[k + 1]]
    single = len(ts) >= 2 and not ts[-2] and ts[-1]
    tail = len(w.ids) - pairs[-1] - 2 if pairs and not single else 0
    return bool(pairs), single, tail


def test_the_cases_meet_the_conditions_together(solved):
    wins = [w for c in solved.values() for w in c.windows]
    assert any(p and not s and tail > 0 and w.advance < WHOLE for w in wins for p, s, tail in [_shape(w)])            # (a)
    assert any(s for w in wins for _, s, _ in [_shape(w)])                                                            # (b)
    assert any(not p for w in wins for p, _, _ in [_shape(w)])                                                        # (c)
    lse = [m for w in wins for m in w.lse_margins if np.isfinite(m)]
    assert any(m > 0 for m in lse) and any(m < 0 for m in lse) and min(abs(m) for m in lse) >= SC.MARGIN              # (d)
    free, bound = solved[("A", "clip(5.0, 2)", -1, 1)], solved[("A", "clip(5.0, 2)", 25, 1)]                          # (e)
    assert free.windows[0].ids[0] - T0 > 25 >= bound.windows[0].ids[0] - T0
    assert {mi for _, _, mi, _ in SC.CASES} == {-1, 25}
    # the re-decoding case: the first window's last pair closes below a whole window, and ids behind it are discarded
    st, cl, mi = SC.REDECODED
    w = solved[(st, cl, mi, 1)].windows[0]
    assert _shape(w)[2] > 0 and 0 < w.advance < WHOLE


def test_the_silence_clip_separates_its_windows(models):
    o = SC.SILENCE
    c = SR.clip_transcribe(models[o["set"]], CFG, SC.speech_then_silence(), SC.SR, 1, o["max_initial"], None, o["no_speech_threshold"], o["logprob_threshold"])
    assert [w.silent for w in c.windows] == [False, True, True] and [w.advance for w in c.windows] == [WHOLE] * 3
    for w in c.windows:                                      # both thresholds decide by far more than the device's error (E: of a log-probability)
        assert np.log(w.no_speech_prob) - np.log(o["no_speech_threshold"]) > 100 * SC.E and abs(w.logprob / w.count - o["logprob_threshold"]) > 100 * SC.E
        assert w.margin >= SC.MARGIN
    alone = SR.clip_transcribe(models[o["set"]], CFG, SC.speech_then_silence()[:2 * SC.SR], SC.SR, 1, o["max_initial"])
    assert c.ids == alone.ids and c.ids and c.segments == alone.segments


# ---------------------------------------------------------------------------------------------- (ii) the step rule
HISTORIES = {"empty": [], "one timestamp": [T0 + 7], "timestamp + text": [T0 + 7, 31], "a closed pair": [T0 + 3, 31, T0 + 20, T0 + 20],
             "a pair followed by text": [T0 + 3, 31, T0 + 20, T0 + 20, 44, 45], "text then a timestamp": [T0, 12, 13, T0 + 50]}


def _processor(max_initial):
    from transformers.generation.logits_process import WhisperTimeStampLogitsProcessor
    gc = types.SimpleNamespace(no_timestamps_token_id=T0 - 1, eos_token_id=EOS, bos_token_id=EOS, _detect_timestamp_from_logprob=True,
                               max_initial_timestamp_index=None if max_initial < 0 else max_initial)
    return WhisperTimeStampLogitsProcessor(gc, begin_index=len(CFG.prefix) - 1)


@pytest.mark.parametrize("name", list(HISTORIES))
@pytest.mark.parametrize("max_initial", [-1, 25])
def test_the_step_rule_is_the_processors(name, max_initial):
    h = HISTORIES[name]
    never, begin = SR.suppress_mask(CFG)
    proc = _processor(max_initial)
    rng = np.random.default_rng(len(name) + max_initial)
    seen = set()
    for trial in range(40):
        lg = rng.normal(0.0, 3.0, size=V).astype(np.float32)
        lg[T0:] += rng.choice([-6.0, -3.0, 0.0, 3.0])        # (so that the logsumexp rule decides both ways over the trials)
        mine, margin = SR.step_row(lg, h, T0, EOS, never, begin, max_initial)
        if abs(margin) < 1e-3:
            continue                                          # (the processor decides in float32)
        given = torch.from_numpy(lg.copy())
        given[torch.from_numpy(never | (begin if not h else np.zeros(V, dtype=bool)))] = -float("inf")
        ids = torch.tensor([SR.ts_prefix(CFG) + h])
        theirs = proc(ids, given[None])[0].double().numpy()
        assert np.array_equal(np.isneginf(theirs), np.isneginf(mine)), (name, trial)
        keep = ~np.isneginf(mine)
        assert np.array_equal(theirs[keep], mine[keep]) and keep.any()
        seen.add(bool(margin > 0))
    # no text may open a window and no timestamp may follow a lone one or a pair: there the decision has one outcome
    assert seen == ({True} if not h else {False} if name in ("one timestamp", "a closed pair") else {True, False}), seen


def test_the_history_state_is_enough():
    """The three facts the device keeps per row - last token a timestamp, the one before it too, the last timestamp id - give the bars
    of the full history, for every history the rule itself can produce (random walks over the allowed ids)."""
    rng = np.random.default_rng(5)
    shapes = set()
    for walk in range(60):
        h = []
        for step in range(12):
            want = SR.step_bars(V, T0, EOS, h, 25 if walk % 2 else -1)
            flags, last = SR.state_of(h, T0)
            assert np.array_equal(SR.bars_from_state(V, T0, CFG.n_timestamps, EOS, flags, last, not h, 25 if walk % 2 else -1), want), h
            shapes.add((flags, last > 0))
            allowed = np.flatnonzero(~want & (np.arange(V) != EOS))
            text, stamps = allowed[allowed < T0], allowed[allowed >= T0]
            pick = stamps if (stamps.size and (not text.size or rng.random() < 0.5)) else text
            if not pick.size:
                break
            h.append(int(rng.choice(pick[:6])))
    assert shapes >= {(2, False), (3, True), (0, True), (1, True)}


# ---------------------------------------------------------------------------------------------- (iii) the seek rule
def _retrieve(seq, offset_ticks, own):
    from transformers.models.whisper.generation_whisper import WhisperGenerationMixin
    segs, adv = WhisperGenerationMixin._retrieve_segment(
        seek_sequence=torch.tensor(seq), seek_outputs=[None], time_offset=torch.tensor([offset_ticks * 0.02], dtype=torch.float64), timestamp_begin=T0,
        seek_num_frames=torch.tensor([2 * own]), time_precision=0.02, time_precision_features=0.01, input_stride=2, prev_idx=0, idx=0,
        return_token_timestamps=False, decoder_input_ids=torch.zeros(1, 3, dtype=torch.long))
    out = [(int(round((float(g["start"]) - offset_ticks * 0.02) / 0.02)), int(round((float(g["end"]) - offset_ticks * 0.02) / 0.02)),
            [int(t) for t in g["tokens"] if int(t) < T0]) for g in segs]
    return out, int(adv) // 2


SEQUENCES = {
    "a pair and a discarded tail": ([T0 + 4, 11, 12, T0 + 40, T0 + 40, 13, 14], 100),
    "two pairs, the second at the end": ([T0 + 4, 11, T0 + 40, T0 + 40, 13, T0 + 90, T0 + 90], 100),
    "pairs whose timestamps differ": ([T0, 11, T0 + 30, T0 + 35, 13, 14, 15], 100),
    "a single trailing timestamp behind a pair": ([T0 + 2, 11, T0 + 40, T0 + 40, 13, T0 + 77], 100),
    "no pair, a trailing timestamp": ([T0 + 2, 11, 12, T0 + 77], 100),
    "no pair, no second timestamp": ([T0 + 2, 11, 12, 13], 100),
    "no pair in a short last window": ([T0, 11, 12], 37),
    "a lone timestamp": ([T0 + 76], 100),
}


@pytest.mark.parametrize("name", list(SEQUENCES))
def test_the_seek_rule_is_retrieve_segment(name):
    seq, own = SEQUENCES[name]
    mine, adv = SR.seek_rule(seq, T0, own, WHOLE)
    theirs, their_adv = _retrieve(seq, 130, own)
    assert mine == theirs, (mine, theirs)
    whole = their_adv == own                                 # (transformers consumes the window's own frames, the restatement a whole window)
    assert adv == (WHOLE if whole else their_adv) and adv > 0
    kinds = {"a pair and a discarded tail": 40, "pairs whose timestamps differ": 30, "two pairs, the second at the end": 90}
    if name in kinds:
        assert adv == kinds[name]


def test_a_window_that_would_not_move_moves_by_a_whole_window():
    segs, adv = SR.seek_rule([T0, 11, T0, T0, 12], T0, 100, WHOLE)
    assert adv == WHOLE and segs == [(0, 0, [11])]


# ---------------------------------------------------------------------------------------------- (iv) the loop
def _hf_long_form(model, x16, max_initial):
    """transformers' own long-form generate on the small configuration: (segments as (start tick, end tick, text ids), all ids)."""
    fe = OW.feature_extractor(CFG)
    feats = fe(x16, sampling_rate=CFG.sample_rate, return_tensors="pt", truncation=False, padding="longest", return_attention_mask=True)
    gc = model.generation_config
    gc.no_timestamps_token_id, gc.lang_to_id, gc.task_to_id, gc.is_multilingual = T0 - 1, {"<|en|>": CFG.prefix[1]}, {"transcribe": CFG.prefix[2]}, True
    gc.suppress_tokens, gc.begin_suppress_tokens = list(range(EOS + 1, T0)), list(CFG.begin_suppress)
    gc.max_initial_timestamp_index = None if max_initial < 0 else max_initial
    gc.eos_token_id, gc.pad_token_id, gc.decoder_start_token_id = EOS, EOS, CFG.prefix[0]
    gc.max_length = len(CFG.prefix) - 1 + SR.budget_of(CFG)
    out = model.generate(feats.input_features, attention_mask=feats.attention_mask, return_timestamps=True, condition_on_prev_tokens=False, num_beams=1,
                         do_sample=False, language="en", task="transcribe", return_segments=True)
    segs = [(int(round(float(g["start"]) / 0.02)), int(round(float(g["end"]) / 0.02)), [int(t) for t in g["tokens"] if int(t) < T0 and int(t) != EOS])
            for g in out["segments"][0]]
    return segs, feats.input_features[0]


@pytest.mark.parametrize("st,seconds,seed,max_initial", [("A", 5.0, 2, 25), ("A", 4.1, 5, -1)])
def test_the_loop_is_transformers_long_form_generate(models, st, seconds, seed, max_initial):
    """transformers' long-form generate(return_timestamps=True, condition_on_prev_tokens=False, num_beams=1) accepts the small
    configuration.  It featurises the whole clip once and slices the features at its seek positions (zero-padded to a window), where
    the native call featurises every window from its own samples; so the restated loop is given transformers' slices as its features,
    and then its greedy ids and segment times are transformers'.  Both cases' windows end on end-of-sequence: transformers' length
    limit is not this path's per-window budget (on set B, whose windows run into the budget, its last window went on to 24 tokens
    where the budget is 12), and the budget is part of neither rule."""
    from tests.test_oracle_whisper import clip
    x16 = clip(seconds, CFG.sample_rate, seed)
    theirs, feats = _hf_long_form(models[st], x16, max_initial)
    tick, frames = int(0.02 * CFG.sample_rate), 2 * CFG.n_ctx

    def sliced(off, n):
        seg = feats[:, 2 * (off // tick):2 * (off // tick) + frames]
        return torch.nn.functional.pad(seg, (0, frames - seg.shape[-1]))
    mine = SR.clip_transcribe(models[st], CFG, x16, CFG.sample_rate, 1, max_initial, features=sliced)
    print(st, seconds, seed, [(w.offset // tick, w.advance, w.ids) for w in mine.windows], f"margin {mine.margin:.3g}")
    assert mine.margin >= 1e-4                               # (transformers decides in float32)
    assert mine.segments == theirs and len(mine.windows) >= 3
    assert mine.ids == sum((t for _, _, t in theirs), [])


# ---------------------------------------------------------------------------------------------- (v) the wrapper
class FakeLib:
    """rt_stt_transcribe_seek with a fixed answer: 2 clips, 3 + 1 segments, 2 + 1 windows, 5 and 1 ids; fills what fits, as the library
    does, and returns RT_ERR_LENGTH when a cap is short."""
    SEGS = [(0, 4, 40, 2), (0, 40, 96, 2), (0, 110, 150, 1), (1, 0, 30, 1)]
    WINS = [(0, 0, 9, -3.0, 0.25, 96), (0, 96 * 480, 5, -2.0, 0.5, 100), (1, 0, 3, -1.0, 0.125, 100)]
    IDS = [[11, 12, 13, 14, 15], [21]]

    def __init__(self):
        self.calls = []

    def rt_stt_transcribe_seek(self, handle, ptrs, lens, n, sr, opts, out):
        o, q = out._obj, opts._obj
        self.calls.append((q.max_tokens, o.segment_cap, o.window_cap, q.beam_size, q.max_initial_timestamp_index, q.no_speech_threshold))
        if o.segment_cap < 1 or o.window_cap < 1:
            return _native.RT_ERR_INVALID
        segs, wins, all_ids = [g for g in self.SEGS if g[0] < n], [w for w in self.WINS if w[0] < n], self.IDS[:n]
        for i, ids in enumerate(all_ids):
            o.h_n_tokens[i] = min(len(ids), q.max_tokens)
            for k in range(o.h_n_tokens[i]):
                o.h_tokens[i * q.max_tokens + k] = ids[k]
            o.h_scores[i], o.h_language[i], o.h_language_prob[i] = -0.5 - i, 292, 1.0
        for g, (c, a, b, k) in enumerate(segs[:o.segment_cap]):
            o.h_seg_clip[g], o.h_seg_start_tick[g], o.h_seg_end_tick[g], o.h_seg_n_ids[g] = c, a, b, k
            o.h_seg_start[g], o.h_seg_end[g] = a * 0.02, b * 0.02
        for w, (c, off, k, lp, ns, adv) in enumerate(wins[:o.window_cap]):
            o.h_win_clip[w], o.h_win_offset[w], o.h_win_n_ids[w], o.h_win_logprob[w], o.h_win_advance[w] = c, off, k, lp, adv
            if o.h_win_no_speech:
                o.h_win_no_speech[w] = ns
        o.n_segments, o.n_windows, o.max_clip_tokens = len(segs), len(wins), max(len(i) for i in all_ids)
        return _native.RT_ERR_LENGTH if len(segs) > o.segment_cap or len(wins) > o.window_cap else _native.RT_OK

    def rt_last_error(self, ctx):
        return b"stand-in"

    def rt_status_string(self, rc):
        return {1: b"invalid argument", 3: b"length"}.get(rc, b"?")


def fake_model(lib=None):
    m = object.__new__(S.NativeSTT)
    m.cfg, m.lib, m.handle = CFG, lib or FakeLib(), 1
    m.ctx = types.SimpleNamespace(check=lambda rc, what: _native.raise_for_status(m.lib, 1, rc, what), device_ordinal=0)
    m._clips = lambda audios: ([torch.zeros(int(a)) for a in audios], len(audios), (C.c_void_p * 2)(), (C.c_int64 * 2)(*[int(a) for a in audios]))
    m.close = lambda: None
    return m


def test_cap_sizing_and_the_one_repeat():
    m = fake_model()
    # 5 s and 0.4 s at 24 kHz with 2-s windows: 2 x 3 + 2 and 2 x 1 + 2 windows, 12 // 2 + 1 segments to a window, 8 x 12 ids
    assert m.seek_caps([5 * SC.SR, int(0.4 * SC.SR)], SC.SR) == (96, 84, 12)
    clips = m.transcribe_ids_seek([5 * SC.SR, int(0.4 * SC.SR)], SC.SR, beam_size=5)
    assert len(m.lib.calls) == 1 and m.lib.calls[0][:4] == (96, 84, 12, 5) and m.lib.calls[0][4] == CFG.max_initial_timestamp_index == 50
    assert np.isnan(m.lib.calls[0][5])
    full = [(c.ids, [(g.start_tick, g.end_tick, g.ids) for g in c.segments], [(w.offset, w.n_ids, w.advance) for w in c.windows]) for c in clips]
    assert full == [([11, 12, 13, 14, 15], [(4, 40, [11, 12]), (40, 96, [13, 14]), (110, 150, [15])], [(0, 9, 96), (96 * 480, 5, 100)]),
                    ([21], [(0, 30, [21])], [(0, 3, 100)])]
    assert clips[0].segments[1].start == pytest.approx(0.8) and clips[0].windows[0].avg_logprob == pytest.approx(-0.3)
    # caps of one: the call is repeated once with the counts it reported, and the result is the full one
    m = fake_model()
    again = m.transcribe_ids_seek([5 * SC.SR, int(0.4 * SC.SR)], SC.SR, caps=(1, 1, 1), max_initial_timestamp_index=-1, no_speech_threshold=0.6)
    assert [c[:3] for c in m.lib.calls] == [(1, 1, 1), (5, 4, 3)] and m.lib.calls[0][4] == -1 and m.lib.calls[0][5] == pytest.approx(0.6)
    assert [(c.ids, len(c.segments), len(c.windows)) for c in again] == [(f[0], len(f[1]), len(f[2])) for f in full]
    # an explicit max_tokens is a cut, not a cap to grow
    m = fake_model()
    cut = m.transcribe_ids_seek([5 * SC.SR, int(0.4 * SC.SR)], SC.SR, max_tokens=3)
    assert len(m.lib.calls) == 1 and [c.ids for c in cut] == [[11, 12, 13], [21]] and [g.ids for g in cut[0].segments] == [[11, 12], [13], []]
    # a library that reports more the second time is an error, not a truncated result
    lib = FakeLib()
    lib.SEGS = FakeLib.SEGS
    m = fake_model(lib)
    real = lib.rt_stt_transcribe_seek

    def growing(*a):
        rc = real(*a)
        a[-1]._obj.n_segments += len(lib.calls)
        return _native.RT_ERR_LENGTH
    lib.rt_stt_transcribe_seek = growing
    with pytest.raises(RuntimeError):
        m.transcribe_ids_seek([5 * SC.SR, int(0.4 * SC.SR)], SC.SR, caps=(1, 1, 1))
    assert len(lib.calls) == 2


def test_wrapper_argument_errors():
    m = fake_model()
    with pytest.raises(ValueError):
        m.transcribe_ids_seek([100], SC.SR, beam_size=9)
    with pytest.raises(ValueError):
        m.transcribe_ids_seek([100], SC.SR, max_tokens=0)
    with pytest.raises(ValueError):
        m.transcribe_ids_seek([100, 100], SC.SR, languages=["en"])
    with pytest.raises(ValueError):                          # a cap of zero is the library's RT_ERR_INVALID
        m.transcribe_ids_seek([100], SC.SR, caps=(4, 0, 4))
    m.cfg = dataclasses.replace(CFG, timestamp_begin=None)
    with pytest.raises(ValueError):
        m.transcribe_ids_seek([100], SC.SR)
    assert not m.lib.calls[1:]


def test_the_join_and_the_construction_errors():
    assert S.join_segment_texts([" Hello there.", " General", ""]) == "Hello there.  General"
    assert S.join_segment_texts([]) == ""
    t = object.__new__(S.WhisperTranscriber)
    t.tokenizer, t.timestamps, t.beam_size, t.auto, t.cfg, t.model = None, True, 1, False, CFG, fake_model()
    assert t.batch([5 * SC.SR, 100], SC.SR) == ["<11> <12> <13> <14> <15>", "<21>"]
    assert t(5 * SC.SR, SC.SR) == "<11> <12> <13> <14> <15>" and t.ids_batch([1, 2], SC.SR) == [[11, 12, 13, 14, 15], [21]]
    assert t.batch_scored([1, 2], SC.SR) == [("<11> <12> <13> <14> <15>", -0.5), ("<21>", -1.5)]
    segs = t.batch_segments([1, 2], SC.SR)
    assert [(g.start_tick, g.end_tick, g.text) for g in segs[0]] == [(4, 40, "<11> <12>"), (40, 96, "<13> <14>"), (110, 150, "<15>")]
    d = t.batch_detailed([1, 2], SC.SR)
    assert (d[0].text, d[0].ids, d[0].language, d[0].windows_dropped, d[0].no_speech_prob) == ("<11> <12> <13> <14> <15>", [11, 12, 13, 14, 15], "en", 0, 0.5)
    t.timestamps = False
    with pytest.raises(ValueError):
        t.batch_segments([1], SC.SR)
    # construction: a configuration without timestamp ids, or whose prefix does not end in <|notimestamps|>
    S.check_timestamp_config(S.tiny_test_config(), False)
    for bad in (S.tiny_test_config(), dataclasses.replace(CFG, prefix=(291, 292, 296)), dataclasses.replace(CFG, vocab=399)):
        with pytest.raises(ValueError):
            S.check_timestamp_config(bad, True)


def test_from_hf_fills_the_timestamp_ids():
    gen = {"no_timestamps_token_id": 50363, "lang_to_id": {"<|en|>": 50259}, "task_to_id": {"transcribe": 50359}, "eos_token_id": 50257,
           "decoder_start_token_id": 50258}
    c = S.SttConfig.from_hf({"vocab_size": 51865}, gen)
    assert c.timestamp_begin == 50364 and c.n_timestamps == 1501 and c.max_initial_timestamp_index == 50 and c.prefix[-1] == 50363
    assert S.SttConfig().timestamp_begin is None
    assert S.SttConfig.from_hf({"vocab_size": 51000}, gen).timestamp_begin is None          # the vocabulary does not hold them
