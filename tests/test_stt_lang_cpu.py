"""Languages and the silence rule of the speech-to-text path, the parts that need no GPU: the configuration (`from_hf`), the
provider's language names, the silence rule, and the float64 restatement of language detection (tests/stt_lang_ref.py) pinned to
transformers' own ``detect_language`` - with the conditions on the cases the GPU tests hold the device to."""
import numpy as np
import pytest

from oracle import whisper as OW
from rho_tts_amd import stt as S
from rho_tts_amd.validation import window_is_silent
from tests import stt_lang_cases as L
from tests import stt_lang_ref as LR
from tests.test_stt_batch_gpu import ragged_clips

WHISPER_TINY = {"d_model": 384, "encoder_attention_heads": 6, "encoder_ffn_dim": 1536, "encoder_layers": 4, "decoder_layers": 4, "num_mel_bins": 80,
                "max_source_positions": 1500, "max_target_positions": 448, "vocab_size": 51865, "eos_token_id": 50257, "decoder_start_token_id": 50258}
GEN = {"lang_to_id": {"<|en|>": 50259, "<|zh|>": 50260, "<|de|>": 50261, "<|ko|>": 50264, "<|ja|>": 50266},
       "task_to_id": {"transcribe": 50359, "translate": 50358}, "no_timestamps_token_id": 50363, "forced_decoder_ids": [[1, None], [2, 50359]]}


def test_from_hf_fills_the_language_fields():
    c = S.SttConfig.from_hf(WHISPER_TINY, GEN)
    assert c.prefix == S.SttConfig().prefix == (50258, 50259, 50359, 50363) and c.language == "en"          # the default: today's prefix
    assert c.languages == {"en": 50259, "zh": 50260, "de": 50261, "ko": 50264, "ja": 50266} and c.no_speech_id == 50362
    zh = S.SttConfig.from_hf(WHISPER_TINY, GEN, language="zh")
    assert zh.prefix == (50258, 50260, 50359, 50363) and zh.language == "zh" and zh.languages == c.languages
    assert zh.max_new_tokens == c.max_new_tokens and zh.begin_suppress == c.begin_suppress
    with pytest.raises(ValueError, match="unknown language"):
        S.SttConfig.from_hf(WHISPER_TINY, GEN, language="xx")
    # a no-timestamps id elsewhere: <|nospeech|> is the id in front of it, as transformers derives it
    assert S.SttConfig.from_hf(WHISPER_TINY, dict(GEN, no_timestamps_token_id=50364)).no_speech_id == 50363
    # the classic multilingual vocabulary without a generation config: the known layout
    k = S.SttConfig.from_hf(WHISPER_TINY)
    assert k == S.SttConfig() and len(k.languages) == 99 and k.no_speech_id == 50362
    assert (k.languages["en"], k.languages["zh"], k.languages["ko"], k.languages["ja"], k.languages["su"]) == (50259, 50260, 50264, 50266, 50357)
    assert sorted(k.languages.values()) == list(range(50259, 50358))
    assert S.SttConfig.from_hf(WHISPER_TINY, language="ja").prefix == (50258, 50266, 50359, 50363)
    # a vocabulary this build knows nothing about has no language slot, and cannot be asked for another language
    other = {"decoder_start_token_id": 900, "vocab_size": 1000, "eos_token_id": 899, "forced_decoder_ids": [[1, None], [2, 905]]}
    assert S.SttConfig.from_hf(other).languages == {} and S.SttConfig.from_hf(other).no_speech_id == -1
    with pytest.raises(ValueError, match="unknown language"):
        S.SttConfig.from_hf(other, language="zh")
    assert S.tiny_test_config().languages == {} and S.tiny_test_config().prefix == (291, 292, 293)


def test_the_classic_codes_are_transformers_own():
    from transformers.models.whisper.tokenization_whisper import LANGUAGES
    assert S.WHISPER_LANGUAGE_CODES == list(LANGUAGES)[:99]


def test_with_language():
    cfg = L.lang_test_config()
    assert cfg.prefix == (291, 292, 296, 298) and cfg.with_language("ko").prefix == (291, 295, 296, 298) and cfg.with_language("ko").language == "ko"
    assert cfg.language_code(294) == "ja" and cfg.language_code(7) is None
    with pytest.raises(ValueError):
        cfg.with_language("de")
    with pytest.raises(ValueError):
        S.tiny_test_config().with_language("en")


def test_whisper_language():
    assert [S.whisper_language(n) for n in ("English", "Chinese", "Japanese", "Korean")] == ["en", "zh", "ja", "ko"]
    assert S.whisper_language("chinese") == S.whisper_language(" CHINESE ") == "zh"
    assert S.whisper_language("de") == "de" and S.whisper_language("ZH") == "zh"
    for bad in ("Klingon", "", "english!", "eng", None, 7):
        with pytest.raises(ValueError):
            S.whisper_language(bad)


@pytest.mark.parametrize("no_speech, avg_logprob, ns_thr, lp_thr, silent", [
    (0.7, -1.5, 0.6, -1.0, True),               # probably silence and low confidence
    (0.7, -0.5, 0.6, -1.0, False),              # probably silence, but decoded with confidence: kept
    (0.5, -1.5, 0.6, -1.0, False),              # low confidence, but not silence
    (0.6, -1.5, 0.6, -1.0, False),              # the comparisons are strict ...
    (0.7, -1.0, 0.6, -1.0, False),              # ... on both sides
    (0.7, -1.5, None, -1.0, False),             # the rule is off
    (0.7, -0.5, 0.6, None, True),               # no log-probability test: the no-speech test alone
    (0.0023, -0.4, 0.002, 0.0, True),           # thresholds of the end-to-end test
    (float("nan"), -1.5, 0.6, -1.0, False),     # no probe ran
    (0.7, float("nan"), 0.6, -1.0, False),
])
def test_the_silence_rule(no_speech, avg_logprob, ns_thr, lp_thr, silent):
    assert window_is_silent(no_speech, avg_logprob, ns_thr, lp_thr) is silent


def test_the_silence_rule_defaults():
    assert window_is_silent(0.7, -1.5) and not window_is_silent(0.7, -0.9) and not window_is_silent(0.59, -1.5)


def test_probe_rule_on_given_logits():
    z = np.full(300, -3.0)
    z[[292, 293, 294, 295]] = [1.0, 2.0, 2.0, 0.5]
    p = LR.probe(z, [295, 294, 293, 292], 297)
    assert p.language == 293 and p.margin == 0.0                                    # two equal maxima: the lowest id
    assert abs(p.log_language_prob - (2.0 - np.log(np.exp([1.0, 2.0, 2.0, 0.5]).sum()))) < 1e-12
    assert abs(p.log_no_speech_prob - (-3.0 - np.log(np.exp(z).sum()))) < 1e-12
    z[293] = np.nan
    assert LR.probe(z, [292, 293, 294, 295], 297).language == 294                   # a NaN never wins
    z = np.full(300, -np.inf)
    z[295] = 0.25
    p = LR.probe(z, [292, 293, 294, 295], 297)
    assert p.language == 295 and p.log_language_prob == 0.0 and p.log_no_speech_prob == -np.inf


@pytest.fixture(scope="module")
def cases():
    """(weight set, clip index, transformers model, first-window log-mel) of every case, and the float64 rule's result."""
    cfg = L.lang_test_config()
    mels = LR.first_window_mels(cfg, ragged_clips(), L.SR)
    out = []
    for name, make in L.STATES.items():
        model = OW.build(cfg, make(cfg))
        out += [(name, i, model, mel, LR.detect(model, cfg, mel)) for i, mel in enumerate(mels)]
    return cfg, out


def test_the_restatement_is_transformers_detect_language(cases):
    cfg, rows = cases
    for name, i, model, mel, want in rows:
        assert LR.hf_detect_language(model, cfg, mel) == want.language, (name, i)


def test_the_conditions_on_the_cases(cases):
    """No case is dropped: every one has a language margin of at least MARGIN, and at least two languages are detected."""
    cfg, rows = cases
    assert len(rows) == 14
    for name, i, _, _, want in rows:
        assert want.margin >= L.MARGIN, (name, i, want.margin)
        assert want.language in cfg.languages.values() and np.isfinite(want.log_language_prob) and np.isfinite(want.log_no_speech_prob)
    assert len({want.language for *_, want in rows}) >= 2
    assert min(want.margin for *_, want in rows) > 0.17                             # the figure stt_lang_cases.py states


class StubSTT:
    """Two clips: one of two windows whose second is silence, one of a single confident window."""

    def __init__(self):
        self.calls = []

    def transcribe_ids_ex(self, audios, sr, beam_size, languages):
        self.calls.append((len(audios), beam_size, languages))
        a = S.SttClip([5, 6, 7, 8], -0.9, 293, 0.7 if languages == "auto" else 1.0, [S.SttWindow(3, -1.2, 0.01), S.SttWindow(1, -4.0, 0.9)])
        b = S.SttClip([9], -0.1, 293, 0.7 if languages == "auto" else 1.0, [S.SttWindow(1, -0.2, 0.95)])
        return [a, b][:len(audios)]

    def transcribe_ids_batch(self, audios, sr):
        self.calls.append(("batch", len(audios)))
        return [[5, 6, 7, 8], [9]][:len(audios)]


def stub_transcriber(**kw):
    tr = object.__new__(S.WhisperTranscriber)
    tr.model, tr.tokenizer, tr.beam_size, tr.cfg = StubSTT(), None, 5, L.lang_test_config().with_language("zh")
    for k, v in kw.items():
        setattr(tr, k, v)
    return tr


def test_the_transcriber_applies_the_silence_rule_on_the_host():
    tr = stub_transcriber(no_speech_threshold=0.6, logprob_threshold=-1.0, _ex=True)
    d = tr.batch_detailed(["a", "b"], 24000)
    assert tr.model.calls == [(2, 5, None)]
    # clip a: the second window (avg -2.0, no-speech 0.9) is silent; clip b: probably silence, but decoded with confidence - kept
    assert (d[0].ids, d[0].text, d[0].windows_dropped, d[0].no_speech_prob) == ([5, 6, 7], "<5> <6> <7>", 1, 0.9)
    assert abs(d[0].avg_logprob - (-1.2 / 4)) < 1e-12 and (d[0].language, d[0].language_prob) == ("zh", 1.0)
    assert (d[1].ids, d[1].windows_dropped, d[1].no_speech_prob) == ([9], 0, 0.95) and abs(d[1].avg_logprob - (-0.1)) < 1e-12
    assert tr.batch(["a", "b"], 24000) == ["<5> <6> <7>", "<9>"] and tr("a", 24000) == "<5> <6> <7>"
    assert tr.batch_scored(["a", "b"], 24000) == [("<5> <6> <7>", d[0].avg_logprob), ("<9>", d[1].avg_logprob)]
    # a fully silent clip is ""
    tr = stub_transcriber(no_speech_threshold=0.005, logprob_threshold=0.0, _ex=True)
    d = tr.batch_detailed(["a"], 24000)[0]
    assert (d.ids, d.text, d.windows_dropped) == ([], "", 2) and abs(d.avg_logprob - (-5.2 / 6)) < 1e-12
    # detection: every call goes through transcribe_ids_ex with "auto"; no threshold: nothing is dropped
    tr = stub_transcriber(auto=True, _ex=True)
    d = tr.batch_detailed(["a", "b"], 24000)
    assert tr.model.calls == [(2, 5, "auto")] and [x.windows_dropped for x in d] == [0, 0] and d[0].ids == [5, 6, 7, 8] and d[0].language_prob == 0.7
    # the defaults: the calls of before
    tr = stub_transcriber()
    tr.beam_size = 1
    assert tr.batch(["a", "b"], 24000) == ["<5> <6> <7> <8>", "<9>"] and tr.model.calls == [("batch", 2)]
