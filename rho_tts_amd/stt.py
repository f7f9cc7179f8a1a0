"""On-GPU speech-to-text for the validation loop: host side of the ``rt_stt_*`` group of the C ABI.

The reference validates a generated segment by writing it to a temporary WAV (base_tts.py:821-830) and transcribing that file
with Whisper "tiny" - faster-whisper on the CPU, or transformers' Whisper (validation/stt/stt_validator.py:42-148).  Here the
waveform never leaves HBM: ``WhisperTranscriber`` is a ``transcriber`` hook of the provider (provider.BatchedPipeline) - a
callable ``(audio, sample_rate) -> text`` - whose model is the hand-written HIP encoder-decoder of ``csrc/stt.hip``.

Weights: a local Whisper checkpoint directory (``model.safetensors`` with transformers' tensor names + ``config.json`` +
``tokenizer.json``) when there is one; there is no network here, so ``openai/whisper-tiny`` cannot be fetched - seeded synthetic
weights of the same architecture serve the parity tests and benchmarks (they transcribe nothing meaningful).
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import json
import math
import os
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _native

DT_BF16, DT_F32 = 0, 1
MAX_BEAM = 8                  # widest beam of rt_stt_transcribe_beam


# The language codes of Whisper's multilingual vocabulary in id order (tokenization_whisper.py LANGUAGES, the first 99: <|en|> is
# 50259, <|su|> 50357), and the ids behind them the classic layout fixes: <|nospeech|> (published as <|nocaptions|>) 50362.
WHISPER_LANGUAGE_CODES = (
    "en zh de es ru ko fr ja pt tr pl ca nl ar sv it id hi fi vi he uk el ms cs ro da hu ta no th ur hr bg lt la mi ml cy sk te fa lv bn sr az sl kn "
    "et mk br eu is hy ne mn bs kk sq sw gl mr pa si km sn yo so af oc ka be tg sd gu am yi lo uz fo ht ps tk nn mt sa lb my bo tl mg as tt haw ln ha "
    "ba jw su").split()
CLASSIC_FIRST_LANGUAGE_ID, CLASSIC_NO_SPEECH_ID = 50259, 50362
CLASSIC_SOT_PREV_ID = 50361              # <|startofprev|> of the same vocabulary
# the languages the provider advertises (provider_info) -> Whisper's codes
_PROVIDER_LANGUAGES = {"english": "en", "chinese": "zh", "japanese": "ja", "korean": "ko"}


def classic_languages() -> Dict[str, int]:
    return {code: CLASSIC_FIRST_LANGUAGE_ID + i for i, code in enumerate(WHISPER_LANGUAGE_CODES)}


def whisper_language(name: str) -> str:
    """The Whisper language code of a language as the provider names it ("Chinese" -> "zh", any case); a two-letter code passes."""
    if not isinstance(name, str):
        raise ValueError(f"language must be a string, got {name!r}")
    key = name.strip().lower()
    if key in _PROVIDER_LANGUAGES:
        return _PROVIDER_LANGUAGES[key]
    if len(key) == 2 and key.isalpha():
        return key
    raise ValueError(f"unknown language {name!r}: one of {sorted(_PROVIDER_LANGUAGES)} or a two-letter code")


def check_beam_size(beam_size) -> int:
    if isinstance(beam_size, bool) or not isinstance(beam_size, (int, np.integer)) or not 1 <= int(beam_size) <= MAX_BEAM:
        raise ValueError(f"beam_size must be an integer in 1 .. {MAX_BEAM}, got {beam_size!r}")
    return int(beam_size)


@dataclass
class SttConfig:
    """Whisper "tiny" (multilingual) by default: models/whisper/configuration_whisper.py of the container's transformers."""
    d_model: int = 384
    heads: int = 6
    ffn: int = 1536
    enc_layers: int = 4
    dec_layers: int = 4
    n_mels: int = 80
    n_ctx: int = 1500
    n_text_ctx: int = 448
    vocab: int = 51865
    n_fft: int = 400
    hop: int = 160
    sample_rate: int = 16000
    chunk_seconds: int = 30
    eos_id: int = 50257
    # <|startoftranscript|> <|en|> <|transcribe|> <|notimestamps|>: what stt_validator.py:137 asks of faster-whisper (language="en")
    prefix: Tuple[int, ...] = (50258, 50259, 50359, 50363)
    suppress_from: int = 50257           # special tokens (language / task / timestamp ids) are never text
    begin_suppress: Tuple[int, ...] = (220, 50257)
    suppress_tokens: Tuple[int, ...] = ()  # further ids never produced (a generation config's `suppress_tokens`)
    max_new_tokens: int = 224
    # the ids position 1 of the prefix may take, by code ("en" -> 50259), and <|nospeech|>: rt_stt_set_languages (empty: a model
    # without a language slot - it transcribes with its prefix as it stands, and nothing can be detected)
    languages: Dict[str, int] = field(default_factory=classic_languages)
    no_speech_id: int = CLASSIC_NO_SPEECH_ID
    language: str = "en"                 # the code position 1 of `prefix` stands for
    # the first timestamp id, <|notimestamps|> + 1 (None: the vocabulary has no timestamp ids this build knows; from_hf fills it):
    # rt_stt_set_timestamps, the seek path (transcribe_ids_seek).  The first token of a window is at most this many ticks of 0.02 s in
    # (1 s, as in openai's and faster-whisper's transcribers; -1: no limit)
    timestamp_begin: Optional[int] = None
    max_initial_timestamp_index: int = 50
    # <|startofprev|>, which opens a window's prompt (NativeSTT.set_prompt; a generation config's `prev_sot_token_id`); None: a
    # vocabulary this build does not know - such a model takes no prompt
    sot_prev_id: Optional[int] = CLASSIC_SOT_PREV_ID
    # word times (NativeSTT.align_ids): the (decoder layer, head) pairs whose cross-attention follows the audio and the width of the
    # median filter along time - a generation config's `alignment_heads` and `median_filter_width`; None: OpenAI's default, every head
    # of the upper half of the decoder layers (``aligned_heads``)
    alignment_heads: Optional[Tuple[Tuple[int, int], ...]] = None
    median_filter_width: int = 7

    @property
    def aligned_heads(self) -> Tuple[Tuple[int, int], ...]:
        """The alignment heads in the order they are averaged in: the configured ones, or every head of the upper half of the decoder."""
        if self.alignment_heads is not None:
            return tuple((int(l), int(h)) for l, h in self.alignment_heads)
        return tuple((l, h) for l in range(self.dec_layers // 2, self.dec_layers) for h in range(self.heads))

    @property
    def n_timestamps(self) -> int:
        """Timestamp ids of one window: <|0.00|> .. <|chunk_seconds|> in ticks of 0.02 s."""
        return int(self.chunk_seconds) * 50 + 1

    def with_language(self, code: str) -> "SttConfig":
        """A copy whose prefix carries ``code`` at position 1."""
        if code not in self.languages or len(self.prefix) < 2:
            raise ValueError(f"unknown language {code!r}: the model knows {sorted(self.languages)}")
        return dataclasses.replace(self, prefix=(self.prefix[0], int(self.languages[code])) + tuple(self.prefix[2:]), language=code)

    def language_code(self, token_id: int) -> Optional[str]:
        return next((k for k, v in self.languages.items() if v == int(token_id)), None)

    @staticmethod
    def from_hf(js: dict, generation: Optional[dict] = None, preprocessor: Optional[dict] = None, language: str = "en") -> "SttConfig":
        """From a checkpoint directory's ``config.json`` (+ ``generation_config.json`` for the forced prefix, the language ids and
        the suppressed ids, + ``preprocessor_config.json`` for the feature extractor), as transformers' ``save_pretrained`` writes
        them.  ``language``: the code position 1 of the prefix is forced to; a code the checkpoint does not know raises."""
        c = SttConfig()
        c.d_model = js.get("d_model", c.d_model)
        c.heads = js.get("encoder_attention_heads", c.heads)
        c.ffn = js.get("encoder_ffn_dim", c.ffn)
        c.enc_layers, c.dec_layers = js.get("encoder_layers", c.enc_layers), js.get("decoder_layers", c.dec_layers)
        c.n_mels, c.n_ctx = js.get("num_mel_bins", c.n_mels), js.get("max_source_positions", c.n_ctx)
        c.n_text_ctx, c.vocab = js.get("max_target_positions", c.n_text_ctx), js.get("vocab_size", c.vocab)
        pre = preprocessor or {}
        c.n_fft, c.hop = int(pre.get("n_fft", c.n_fft)), int(pre.get("hop_length", c.hop))
        c.sample_rate, c.n_mels = int(pre.get("sampling_rate", c.sample_rate)), int(pre.get("feature_size", c.n_mels))
        # the encoder's two convolutions halve the frames: one chunk is 2 n_ctx hops (30 s for n_ctx 1500)
        c.chunk_seconds = int(pre.get("chunk_length", max(1, round(2 * c.n_ctx * c.hop / c.sample_rate))))
        gen = dict(js)
        gen.update({k: v for k, v in (generation or {}).items() if v is not None})
        eos = gen.get("eos_token_id", c.eos_id)
        c.eos_id = int(eos[0] if isinstance(eos, (list, tuple)) else eos)
        start = int(gen.get("decoder_start_token_id", c.prefix[0]))
        # Forced prefix.  The reference transcribes with language="en" (stt_validator.py:137), so position 1 is <|en|> whatever the
        # checkpoint's default is.  Published generation configs carry `forced_decoder_ids: [[1, null], [2, 50359]]` - a None means
        # "decided at generation time", not "absent" - next to lang_to_id / task_to_id / no_timestamps_token_id: a None (or missing)
        # position is filled from those, and the ids they name win over stale forced entries.
        forced = {int(p_): (None if t is None else int(t)) for p_, t in (gen.get("forced_decoder_ids") or [])}
        lang, task = gen.get("lang_to_id") or {}, gen.get("task_to_id") or {}
        nts = gen.get("no_timestamps_token_id")
        if forced or (lang and task):
            classic = start == SttConfig.prefix[0]                  # the multilingual vocabulary the defaults describe
            en = lang.get("<|en|>", forced.get(1))
            if en is None and classic:
                en = SttConfig.prefix[1]
            tr = task.get("transcribe", forced.get(2))
            if tr is None and classic:
                tr = SttConfig.prefix[2]
            nt = nts if nts is not None else forced.get(3)
            if nt is None and classic:
                nt = SttConfig.prefix[3]
            c.prefix = (start,) + tuple(int(t) for t in (en, tr, nt) if t is not None)
        elif start != c.prefix[0]:
            c.prefix = (start,)
        # Language ids and <|nospeech|>: lang_to_id with "<|xx|>" stripped to "xx", and no_timestamps_token_id - 1 as transformers
        # derives it (generation_whisper.py, WhisperNoSpeechDetection's no_speech_token); without a generation config the classic
        # multilingual vocabulary has the known layout (the defaults), and any other vocabulary has no language slot this build knows
        if lang:
            c.languages = {str(k).strip("<|>"): int(v) for k, v in lang.items() if 0 <= int(v) < c.vocab}
            c.no_speech_id = int(nts) - 1 if nts is not None and 0 < int(nts) <= c.vocab else -1
        elif not (start == SttConfig.prefix[0] and c.vocab > CLASSIC_NO_SPEECH_ID):
            c.languages, c.no_speech_id = {}, -1
        # timestamp ids follow <|notimestamps|>; the seek path needs the prefix to end in it and the vocabulary to hold them
        if nts is not None and len(c.prefix) > 1 and c.prefix[-1] == int(nts) and int(nts) + 1 + c.n_timestamps <= c.vocab and c.eos_id < int(nts):
            c.timestamp_begin = int(nts) + 1
        prev = gen.get("prev_sot_token_id")
        if prev is not None and c.eos_id < int(prev) < c.vocab:
            c.sot_prev_id = int(prev)
        elif not (start == SttConfig.prefix[0] and c.vocab > CLASSIC_SOT_PREV_ID):
            c.sot_prev_id = None
        if language != "en":
            c = c.with_language(language)
        elif len(c.prefix) > 1:
            c.language = c.language_code(c.prefix[1]) or "en"
        if gen.get("alignment_heads"):
            c.alignment_heads = tuple((int(l), int(h)) for l, h in gen["alignment_heads"])
        if gen.get("median_filter_width"):
            c.median_filter_width = int(gen["median_filter_width"])
        if gen.get("begin_suppress_tokens"):
            c.begin_suppress = tuple(int(t) for t in gen["begin_suppress_tokens"] if 0 <= int(t) < c.vocab)[:4]
        # Whisper's vocabularies put every special id (language, task, timestamps) behind end-of-sequence
        c.suppress_from = c.eos_id if 0 < c.eos_id < c.vocab else 0
        # `suppress_tokens`: ids never produced (punctuation-only / non-speech tokens and a few specials below end-of-sequence)
        c.suppress_tokens = tuple(int(t) for t in (gen.get("suppress_tokens") or []) if 0 <= int(t) < c.vocab and int(t) != c.eos_id)
        if gen.get("max_new_tokens"):
            c.max_new_tokens = int(gen["max_new_tokens"])
        c.max_new_tokens = max(1, min(c.max_new_tokens, c.n_text_ctx - len(c.prefix)))
        return c

    @staticmethod
    def from_dir(model_dir: str, language: str = "en") -> "SttConfig":
        def read(name):
            path = os.path.join(model_dir, name)
            if not os.path.exists(path):
                return None
            with open(path) as f:
                return json.load(f)
        js = read("config.json")
        if js is None:
            raise ValueError(f"no config.json in {model_dir!r}")
        return SttConfig.from_hf(js, read("generation_config.json"), read("preprocessor_config.json"), language)


def tiny_test_config() -> SttConfig:
    """A few-thousand-parameter model of the same topology for quick tests (2-s chunks)."""
    return SttConfig(d_model=64, heads=2, ffn=128, enc_layers=2, dec_layers=2, n_mels=16, n_ctx=100, n_text_ctx=32, vocab=300,
                     chunk_seconds=2, eos_id=290, prefix=(291, 292, 293), suppress_from=290, begin_suppress=(7, 290), max_new_tokens=12,
                     languages={}, no_speech_id=-1, sot_prev_id=None)


class RtSttConfig(C.Structure):
    _fields_ = [("d_model", C.c_int32), ("heads", C.c_int32), ("ffn", C.c_int32), ("enc_layers", C.c_int32), ("dec_layers", C.c_int32),
                ("n_mels", C.c_int32), ("n_ctx", C.c_int32), ("n_text_ctx", C.c_int32), ("vocab", C.c_int32),
                ("n_fft", C.c_int32), ("hop", C.c_int32), ("sample_rate", C.c_int32), ("chunk_seconds", C.c_int32),
                ("eos_id", C.c_int32), ("n_prefix", C.c_int32), ("prefix", C.c_int32 * 8), ("suppress_from", C.c_int32),
                ("n_begin_suppress", C.c_int32), ("begin_suppress", C.c_int32 * 4), ("max_new_tokens", C.c_int32), ("reserved", C.c_int32 * 4)]


class RtSttDecodeOpts(C.Structure):
    _fields_ = [("h_language", C.POINTER(C.c_int32)), ("beam_size", C.c_int32), ("max_tokens", C.c_int32), ("reserved", C.c_int32 * 4)]


class RtSttDecodeOut(C.Structure):
    _fields_ = [("h_tokens", C.POINTER(C.c_int32)), ("h_n_tokens", C.POINTER(C.c_int32)), ("h_scores", C.POINTER(C.c_float)),
                ("h_language", C.POINTER(C.c_int32)), ("h_language_prob", C.POINTER(C.c_float)), ("h_win_clip", C.POINTER(C.c_int32)),
                ("h_win_n_ids", C.POINTER(C.c_int32)), ("h_win_logprob", C.POINTER(C.c_float)), ("h_win_no_speech", C.POINTER(C.c_float)),
                ("window_cap", C.c_int32), ("n_windows", C.c_int32), ("reserved", C.c_int32 * 4)]


class RtSttSeekOpts(C.Structure):
    _fields_ = [("h_language", C.POINTER(C.c_int32)), ("beam_size", C.c_int32), ("max_tokens", C.c_int32), ("max_initial_timestamp_index", C.c_int32),
                ("no_speech_threshold", C.c_float), ("logprob_threshold", C.c_float), ("reserved", C.c_int32 * 3)]


class RtSttSeekOut(C.Structure):
    _fields_ = [("h_tokens", C.POINTER(C.c_int32)), ("h_n_tokens", C.POINTER(C.c_int32)), ("h_scores", C.POINTER(C.c_float)),
                ("h_language", C.POINTER(C.c_int32)), ("h_language_prob", C.POINTER(C.c_float)),
                ("h_seg_clip", C.POINTER(C.c_int32)), ("h_seg_start", C.POINTER(C.c_float)), ("h_seg_end", C.POINTER(C.c_float)),
                ("h_seg_start_tick", C.POINTER(C.c_int32)), ("h_seg_end_tick", C.POINTER(C.c_int32)), ("h_seg_n_ids", C.POINTER(C.c_int32)),
                ("h_win_clip", C.POINTER(C.c_int32)), ("h_win_offset", C.POINTER(C.c_int64)), ("h_win_n_ids", C.POINTER(C.c_int32)),
                ("h_win_logprob", C.POINTER(C.c_float)), ("h_win_no_speech", C.POINTER(C.c_float)), ("h_win_advance", C.POINTER(C.c_int32)),
                ("segment_cap", C.c_int32), ("window_cap", C.c_int32), ("n_segments", C.c_int32), ("n_windows", C.c_int32),
                ("max_clip_tokens", C.c_int32), ("reserved", C.c_int32 * 3)]


RATIO_FN = C.CFUNCTYPE(C.c_float, C.POINTER(C.c_int32), C.c_int32, C.c_void_p)     # rt_stt_ratio_fn
MAX_TEMPERATURES = 8


class RtSttFallback(C.Structure):
    _fields_ = [("n_temperatures", C.c_int32), ("temperatures", C.c_float * 8), ("best_of", C.c_int32), ("compression_ratio_threshold", C.c_float),
                ("logprob_threshold", C.c_float), ("no_speech_threshold", C.c_float), ("seed", C.c_uint64), ("ratio", RATIO_FN), ("ratio_user", C.c_void_p),
                ("reserved", C.c_int32 * 4)]


class RtSttPrompt(C.Structure):
    _fields_ = [("sot_prev_id", C.c_int32), ("condition_on_previous", C.c_int32), ("reset_on_temperature", C.c_float), ("h_initial", C.POINTER(C.c_int32)),
                ("n_initial", C.c_int32), ("reserved", C.c_int32 * 4)]


class RtSttAlignOut(C.Structure):
    _fields_ = [("h_token_frame", C.POINTER(C.c_int32)), ("h_token_logprob", C.POINTER(C.c_float)), ("h_n_frames", C.POINTER(C.c_int32)),
                ("reserved", C.c_int32 * 4)]


@dataclass
class SttPromptWindow:
    """One window's line of ``NativeSTT.prompt_report``: the length of the prompt it decoded behind, and whether the clip's reset mark
    moved behind it (the next window then starts from an empty prompt)."""
    prompt_len: int
    reset: bool


def check_prompt_args(cfg: "SttConfig", initial_ids, condition_on_previous, reset_on_temperature) -> Tuple[List[int], Optional[float]]:
    """The argument rules of ``NativeSTT.set_prompt``, before anything touches a device: (initial ids, reset temperature)."""
    if cfg.timestamp_begin is None:
        raise ValueError("set_prompt: the configuration has no timestamp ids (SttConfig.timestamp_begin): a prompt applies to the seek path only")
    if cfg.sot_prev_id is None or not cfg.eos_id < int(cfg.sot_prev_id) < cfg.vocab:
        raise ValueError(f"set_prompt: the configuration has no <|startofprev|> id (SttConfig.sot_prev_id = {cfg.sot_prev_id!r})")
    if isinstance(initial_ids, (str, bytes)):
        raise ValueError("set_prompt: initial_ids are token ids (WhisperTranscriber(initial_prompt=...) takes a string)")
    ids = [] if initial_ids is None else list(initial_ids)
    if any(isinstance(t, bool) or not isinstance(t, (int, np.integer)) or not 0 <= int(t) < cfg.vocab for t in ids):
        raise ValueError(f"set_prompt: initial ids must be integers in [0, {cfg.vocab})")
    if not condition_on_previous and not ids:
        raise ValueError("set_prompt: a policy either conditions on previous text or carries an initial prompt")
    if reset_on_temperature is not None and not (float(reset_on_temperature) >= 0.0 and math.isfinite(float(reset_on_temperature))):
        raise ValueError(f"set_prompt: reset_on_temperature must be None or a finite value >= 0, got {reset_on_temperature!r}")
    return [int(t) for t in ids], None if reset_on_temperature is None else float(reset_on_temperature)


def check_temperatures(temperatures) -> Tuple[float, ...]:
    """The temperatures of a fallback policy: 1 .. 8 finite values >= 0, strictly ascending (so only the first may be 0)."""
    ts = tuple(float(t) for t in ((temperatures,) if isinstance(temperatures, (int, float)) else temperatures))
    if not 1 <= len(ts) <= MAX_TEMPERATURES or any(not (t >= 0.0 and math.isfinite(t)) for t in ts) or any(b <= a for a, b in zip(ts, ts[1:])):
        raise ValueError(f"temperatures must be 1 .. {MAX_TEMPERATURES} finite values >= 0 in strictly ascending order, got {temperatures!r}")
    return ts


@dataclass
class SttFallbackWindow:
    """One window's line of ``NativeSTT.fallback_report``: the attempts made, the temperature of the chosen one and its compression
    ratio (NaN when the policy has no ratio callback)."""
    attempts: int
    temperature: float
    compression_ratio: float


FRAME_SECONDS = 0.02           # one frame of the alignment: two log-mel hops, the tick of the timestamp ids


@dataclass
class SttTokenTimes:
    """One window of ``NativeSTT.align_ids``: per text id its start and end in seconds of the window and its log-probability (log_softmax
    over the text ids of the logits that predict it), and the window's frames."""
    start: List[float]
    end: List[float]
    logprob: List[float]
    n_frames: int


@dataclass
class SttWord:
    """One word of a segment or of an aligned text: start and end in seconds, ``probability`` = exp(mean log-probability of its ids),
    and ``ids``, the token ids it was grouped from (a segment's words hold the segment's ids in order; beyond faster-whisper's ``Word``)."""
    word: str
    start: float
    end: float
    probability: float
    ids: List[int] = field(default_factory=list)


@dataclass
class SttSegment:
    """One closed segment of a clip (transcribe_ids_seek): start and end in seconds of the clip (and in ticks of 0.02 s, which is what
    the decoder's timestamp ids count), and its text ids."""
    start: float
    end: float
    ids: List[int]
    start_tick: int = 0
    end_tick: int = 0
    text: Optional[str] = None           # WhisperTranscriber.batch_segments fills it
    # under a fallback policy (WhisperTranscriber(temperatures=...)), of the window that closed the segment
    temperature: float = 0.0
    attempts: int = 1
    compression_ratio: float = float("nan")
    prompt_len: int = 0                  # under a prompt policy, of the window that closed the segment
    words: Optional[List[SttWord]] = None    # WhisperTranscriber(word_timestamps=True).batch_segments fills it


@dataclass
class SttSeekWindow:
    """One decoded window of a clip on the seek path: where it started (input samples), what it decoded (timestamp ids counted) and how
    far it moved the clip on (ticks)."""
    offset: int
    n_ids: int
    logprob: float
    no_speech_prob: float                # NaN where the probe pass did not run
    advance: int
    prompt_len: int = 0                  # under a prompt policy (NativeSTT.set_prompt): the ids of previous text it decoded behind

    @property
    def avg_logprob(self) -> float:
        return self.logprob / (self.n_ids + 1)


@dataclass
class SttSeekClip:
    """One clip of ``NativeSTT.transcribe_ids_seek``: ``SttClip`` with the closed segments and the windows of the seek path."""
    ids: List[int]
    score: float
    language: int
    language_prob: float
    segments: List[SttSegment]
    windows: List[SttSeekWindow]


@dataclass
class SttWindow:
    """One chunk_seconds window of a clip as rt_stt_transcribe_ex reports it."""
    n_ids: int
    logprob: float                       # cumulative log-probability of the window's hypothesis, end-of-sequence counted
    no_speech_prob: float                # NaN where the probe pass did not run

    @property
    def avg_logprob(self) -> float:
        return self.logprob / (self.n_ids + 1)


@dataclass
class SttClip:
    """One clip of ``NativeSTT.transcribe_ids_ex``: ``language`` is the id at position 1 of its prefix, ``language_prob`` its
    probability among the configured ids where it was detected and 1 where it was given."""
    ids: List[int]
    score: float
    language: int
    language_prob: float
    windows: List[SttWindow]


def _rt_config(c: SttConfig) -> RtSttConfig:
    r = RtSttConfig()
    for k in ("d_model", "heads", "ffn", "enc_layers", "dec_layers", "n_mels", "n_ctx", "n_text_ctx", "vocab", "n_fft", "hop", "sample_rate",
              "chunk_seconds", "eos_id", "suppress_from", "max_new_tokens"):
        setattr(r, k, int(getattr(c, k)))
    r.n_prefix = len(c.prefix)
    for i, t in enumerate(c.prefix):
        r.prefix[i] = int(t)
    r.n_begin_suppress = len(c.begin_suppress)
    for i, t in enumerate(c.begin_suppress):
        r.begin_suppress[i] = int(t)
    return r


_DECLARED = False


def _declare(lib: C.CDLL) -> None:
    global _DECLARED
    if _DECLARED:
        return
    vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    lib.rt_stt_create.argtypes = [vp, C.POINTER(RtSttConfig), C.POINTER(vp)]
    lib.rt_stt_destroy.argtypes = [vp]
    lib.rt_stt_tensor_count.argtypes = [vp]
    lib.rt_stt_tensor_info.argtypes = [vp, i32, C.c_char_p, C.c_size_t, C.POINTER(i64), C.POINTER(i32)]
    lib.rt_stt_set_tensor.argtypes = [vp, C.c_char_p, vp, i32, i64, i64, i32]
    lib.rt_stt_finalize.argtypes = [vp]
    lib.rt_stt_set_suppress.argtypes = [vp, C.POINTER(i32), i32]
    lib.rt_stt_transcribe.argtypes = [vp, vp, i64, i32, C.POINTER(i32), i32, C.POINTER(i32), vp]
    lib.rt_stt_transcribe_batch.argtypes = [vp, C.POINTER(vp), C.POINTER(i64), i32, i32, C.POINTER(i32), i32, C.POINTER(i32)]
    lib.rt_stt_transcribe_beam.argtypes = [vp, C.POINTER(vp), C.POINTER(i64), i32, i32, i32, C.POINTER(i32), i32, C.POINTER(i32), C.POINTER(C.c_float)]
    lib.rt_stt_set_languages.argtypes = [vp, C.POINTER(i32), i32, i32]
    lib.rt_stt_detect_language.argtypes = [vp, C.POINTER(vp), C.POINTER(i64), i32, i32, C.POINTER(i32), C.POINTER(C.c_float), C.POINTER(C.c_float)]
    lib.rt_stt_transcribe_ex.argtypes = [vp, C.POINTER(vp), C.POINTER(i64), i32, i32, C.POINTER(RtSttDecodeOpts), C.POINTER(RtSttDecodeOut)]
    lib.rt_stt_set_timestamps.argtypes = [vp, i32, i32]
    lib.rt_stt_transcribe_seek.argtypes = [vp, C.POINTER(vp), C.POINTER(i64), i32, i32, C.POINTER(RtSttSeekOpts), C.POINTER(RtSttSeekOut)]
    lib.rt_stt_set_fallback.argtypes = [vp, C.POINTER(RtSttFallback)]
    lib.rt_stt_fallback_report.argtypes = [vp, i32, C.POINTER(i32), C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(i32)]
    lib.rt_stt_set_prompt.argtypes = [vp, C.POINTER(RtSttPrompt)]
    lib.rt_stt_prompt_report.argtypes = [vp, i32, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]
    lib.rt_stt_set_alignment.argtypes = [vp, C.POINTER(i32), i32, i32]
    lib.rt_stt_align.argtypes = [vp, C.POINTER(vp), C.POINTER(i64), i32, i32, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32), C.POINTER(RtSttAlignOut)]
    lib.rt_stt_log_mel.argtypes = [vp, vp, i64, i32, vp]
    lib.rt_stt_encode.argtypes = [vp, vp, i64, i32, vp]
    _DECLARED = True


# ---------------------------------------------------------------------------------------------- front-end constants
def hertz_to_mel_slaney(f):
    f = np.asarray(f, dtype=np.float64)
    mels = 3.0 * f / 200.0
    log = f >= 1000.0
    return np.where(log, 15.0 + np.log(np.maximum(f, 1e-30) / 1000.0) * (27.0 / np.log(6.4)), mels)


def mel_to_hertz_slaney(m):
    m = np.asarray(m, dtype=np.float64)
    f = 200.0 * m / 3.0
    log = m >= 15.0
    return np.where(log, 1000.0 * np.exp((np.log(6.4) / 27.0) * (m - 15.0)), f)


def mel_filters(n_fft: int, n_mels: int, sample_rate: int, f_max: float = 8000.0) -> np.ndarray:
    """[n_fft // 2 + 1][n_mels] float32 slaney-normalised triangular filters: what WhisperFeatureExtractor builds with
    transformers.audio_utils.mel_filter_bank(..., norm="slaney", mel_scale="slaney") (feature_extraction_whisper.py:95-103)."""
    n_bins = n_fft // 2 + 1
    mel_pts = np.linspace(hertz_to_mel_slaney(0.0), hertz_to_mel_slaney(f_max), n_mels + 2)
    hz = mel_to_hertz_slaney(mel_pts)
    fft_freqs = np.linspace(0, sample_rate // 2, n_bins)
    diff = np.diff(hz)
    slopes = hz[None, :] - fft_freqs[:, None]
    down = -slopes[:, :-2] / diff[:-1]
    up = slopes[:, 2:] / diff[1:]
    fb = np.maximum(0.0, np.minimum(down, up))
    fb *= (2.0 / (hz[2: n_mels + 2] - hz[:n_mels]))[None, :]
    return fb.astype(np.float32)


def hann_window(n_fft: int) -> np.ndarray:
    """torch.hann_window(n_fft) (periodic) in float32."""
    return torch.hann_window(n_fft, periodic=True, dtype=torch.float32).numpy()


# ---------------------------------------------------------------------------------------------- weights
def tensor_specs(c: SttConfig) -> List[Tuple[str, Tuple[int, ...], str, float]]:
    """(name, shape, kind, scale) with transformers' Whisper tensor names (models/whisper/modeling_whisper.py)."""
    D, F = c.d_model, c.ffn
    s: List[Tuple[str, Tuple[int, ...], str, float]] = [
        ("model.encoder.conv1.weight", (D, c.n_mels, 3), "fan", 1.0), ("model.encoder.conv1.bias", (D,), "bias", 0.01),
        ("model.encoder.conv2.weight", (D, D, 3), "fan", 1.0), ("model.encoder.conv2.bias", (D,), "bias", 0.01),
        ("model.encoder.embed_positions.weight", (c.n_ctx, D), "mat", 0.02)]

    def layer(p: str, cross: bool):
        out = []
        blocks = [("self_attn", "self_attn_layer_norm")] + ([("encoder_attn", "encoder_attn_layer_norm")] if cross else [])
        for att, ln in blocks:
            out += [(f"{p}.{att}.k_proj.weight", (D, D), "mat", 0.05), (f"{p}.{att}.v_proj.weight", (D, D), "mat", 0.05),
                    (f"{p}.{att}.v_proj.bias", (D,), "bias", 0.01), (f"{p}.{att}.q_proj.weight", (D, D), "mat", 0.05),
                    (f"{p}.{att}.q_proj.bias", (D,), "bias", 0.01), (f"{p}.{att}.out_proj.weight", (D, D), "mat", 0.05),
                    (f"{p}.{att}.out_proj.bias", (D,), "bias", 0.01), (f"{p}.{ln}.weight", (D,), "norm", 0.1), (f"{p}.{ln}.bias", (D,), "bias", 0.02)]
        out += [(f"{p}.fc1.weight", (F, D), "mat", 0.05), (f"{p}.fc1.bias", (F,), "bias", 0.01), (f"{p}.fc2.weight", (D, F), "mat", 0.03),
                (f"{p}.fc2.bias", (D,), "bias", 0.01), (f"{p}.final_layer_norm.weight", (D,), "norm", 0.1), (f"{p}.final_layer_norm.bias", (D,), "bias", 0.02)]
        return out
    for i in range(c.enc_layers):
        s += layer(f"model.encoder.layers.{i}", False)
    s += [("model.encoder.layer_norm.weight", (D,), "norm", 0.1), ("model.encoder.layer_norm.bias", (D,), "bias", 0.02),
          ("model.decoder.embed_tokens.weight", (c.vocab, D), "mat", 0.05), ("model.decoder.embed_positions.weight", (c.n_text_ctx, D), "mat", 0.02)]
    for i in range(c.dec_layers):
        s += layer(f"model.decoder.layers.{i}", True)
    s += [("model.decoder.layer_norm.weight", (D,), "norm", 0.1), ("model.decoder.layer_norm.bias", (D,), "bias", 0.02)]
    return s


def synthetic_state(c: SttConfig, seed: int = 789, device="cpu") -> Dict[str, torch.Tensor]:
    """Seeded bf16-valued weights (the counter-hash generator of weights.py: the same bytes on CPU and GPU)."""
    from .weights import synth_tensor
    return {sp[0]: synth_tensor(sp, None, seed, device) for sp in tensor_specs(c)}


def load_checkpoint(c: SttConfig, model_dir: str, device="cpu") -> Dict[str, torch.Tensor]:
    """``*.safetensors`` of a local Whisper checkpoint (transformers' names); nothing is executed from the files."""
    from safetensors import safe_open
    want = {sp[0]: sp[1] for sp in tensor_specs(c)}
    state: Dict[str, torch.Tensor] = {}
    files = [os.path.join(model_dir, f) for f in sorted(os.listdir(model_dir)) if f.endswith(".safetensors")]
    if not files:
        raise FileNotFoundError(f"no .safetensors files in {model_dir}")
    for path in files:
        with safe_open(path, framework="pt", device=str(device)) as sf:
            for k in sf.keys():
                name = k if k in want else ("model." + k if "model." + k in want else None)
                if name is None:
                    continue
                t = sf.get_tensor(k)
                if tuple(t.shape) != tuple(want[name]):
                    raise ValueError(f"{k}: checkpoint shape {tuple(t.shape)} != configured {want[name]}")
                state[name] = t
    missing = sorted(set(want) - set(state))
    if missing:
        raise ValueError(f"Whisper checkpoint is missing {len(missing)} of {len(want)} tensors, e.g. {missing[:4]}")
    return state


def to_native(state: Dict[str, torch.Tensor], c: SttConfig) -> Dict[str, torch.Tensor]:
    """transformers' names / layouts -> the library's tensors (bf16 matrices [N][K], float32 vectors):
    Conv1d k3 [Co][Ci][3] -> [Co][tap * Ci + ci];  the stride-2 conv over rows [x[2t], x[2t+1]] -> [Co][0 | W0 | W1 | W2];
    q / k / v projections concatenated ([3D][D]; k_proj has no bias: zeros), cross-attention k / v likewise ([2D][D])."""
    bf, D = torch.bfloat16, c.d_model
    out: Dict[str, torch.Tensor] = {}

    def f32(t):
        return t.detach().to(torch.float32).contiguous()

    def mat(t):
        return t.detach().to(bf).contiguous()
    w1 = state["model.encoder.conv1.weight"]
    out["enc.conv1"] = mat(w1.permute(0, 2, 1).reshape(D, -1))
    out["enc.conv1_b"] = f32(state["model.encoder.conv1.bias"])
    w2 = state["model.encoder.conv2.weight"].to(torch.float32)                  # [Co][Ci][3]
    z = torch.zeros(D, D, dtype=torch.float32, device=w2.device)
    out["enc.conv2"] = mat(torch.cat([z, w2[:, :, 0], w2[:, :, 1], w2[:, :, 2]], dim=1))
    out["enc.conv2_b"] = f32(state["model.encoder.conv2.bias"])
    out["enc.pos"] = f32(state["model.encoder.embed_positions.weight"]).reshape(-1)

    def layer(src: str, dst: str, cross: bool):
        a = f"{src}.self_attn"
        zb = torch.zeros(D, dtype=torch.float32, device=state[f"{a}.q_proj.bias"].device)
        out[f"{dst}.ln1_w"], out[f"{dst}.ln1_b"] = f32(state[f"{src}.self_attn_layer_norm.weight"]), f32(state[f"{src}.self_attn_layer_norm.bias"])
        out[f"{dst}.wqkv"] = mat(torch.cat([state[f"{a}.q_proj.weight"], state[f"{a}.k_proj.weight"], state[f"{a}.v_proj.weight"]], 0))
        out[f"{dst}.bqkv"] = torch.cat([f32(state[f"{a}.q_proj.bias"]), zb, f32(state[f"{a}.v_proj.bias"])])
        out[f"{dst}.wo"], out[f"{dst}.bo"] = mat(state[f"{a}.out_proj.weight"]), f32(state[f"{a}.out_proj.bias"])
        if cross:
            e = f"{src}.encoder_attn"
            out[f"{dst}.lnc_w"], out[f"{dst}.lnc_b"] = f32(state[f"{src}.encoder_attn_layer_norm.weight"]), f32(state[f"{src}.encoder_attn_layer_norm.bias"])
            out[f"{dst}.cwq"], out[f"{dst}.cbq"] = mat(state[f"{e}.q_proj.weight"]), f32(state[f"{e}.q_proj.bias"])
            out[f"{dst}.cwkv"] = mat(torch.cat([state[f"{e}.k_proj.weight"], state[f"{e}.v_proj.weight"]], 0))
            out[f"{dst}.cbkv"] = torch.cat([zb, f32(state[f"{e}.v_proj.bias"])])
            out[f"{dst}.cwo"], out[f"{dst}.cbo"] = mat(state[f"{e}.out_proj.weight"]), f32(state[f"{e}.out_proj.bias"])
        out[f"{dst}.ln2_w"], out[f"{dst}.ln2_b"] = f32(state[f"{src}.final_layer_norm.weight"]), f32(state[f"{src}.final_layer_norm.bias"])
        out[f"{dst}.fc1"], out[f"{dst}.fc1_b"] = mat(state[f"{src}.fc1.weight"]), f32(state[f"{src}.fc1.bias"])
        out[f"{dst}.fc2"], out[f"{dst}.fc2_b"] = mat(state[f"{src}.fc2.weight"]), f32(state[f"{src}.fc2.bias"])
    for i in range(c.enc_layers):
        layer(f"model.encoder.layers.{i}", f"enc.l{i}", False)
    out["enc.ln_w"], out["enc.ln_b"] = f32(state["model.encoder.layer_norm.weight"]), f32(state["model.encoder.layer_norm.bias"])
    out["dec.tok"] = mat(state["model.decoder.embed_tokens.weight"])
    out["dec.pos"] = f32(state["model.decoder.embed_positions.weight"]).reshape(-1)
    for i in range(c.dec_layers):
        layer(f"model.decoder.layers.{i}", f"dec.l{i}", True)
    out["dec.ln_w"], out["dec.ln_b"] = f32(state["model.decoder.layer_norm.weight"]), f32(state["model.decoder.layer_norm.bias"])
    out["fe.window"] = torch.from_numpy(hann_window(c.n_fft))
    out["fe.melT"] = torch.from_numpy(mel_filters(c.n_fft, c.n_mels, c.sample_rate)).reshape(-1)
    return out


def _i32(k: int):
    return (C.c_int32 * max(k, 1))()


def _f32(k: int):
    return (C.c_float * max(k, 1))()


def _clip_ids(toks, counts, n: int, cap: int) -> List[List[int]]:
    """The ids of ``n`` clips out of ``toks`` [n][cap], ``counts[i]`` of clip i."""
    return [[int(toks[i * cap + k]) for k in range(counts[i])] for i in range(n)]


# ---------------------------------------------------------------------------------------------- word grouping (host, no GPU)
# OpenAI's rules (whisper/tokenizer.py split_tokens_on_unicode / split_tokens_on_spaces, whisper/timing.py merge_punctuations) restated
# over a ``decode(ids) -> str`` callable that renders ids as they are (no special id skipped).  A group is (text, positions): the
# positions index the ids that were passed in, so a caller looks the group's times up by position.  OpenAI's word-duration clamps and
# its hallucination_silence_threshold are not restated ("word times").
PREPEND_PUNCTUATIONS = "\"'“¿([{-"
APPEND_PUNCTUATIONS = "\"'.。,，!！?？:：”)]}、"
_PUNCTUATION = "!\"#$%&'()*+,-./:;<=>?@[\\]^_`{|}~"          # string.punctuation
UNSPACED_LANGUAGES = ("zh", "ja", "th", "lo", "my", "yue")     # written without spaces: every decodable piece is a word


def split_tokens_on_unicode(ids: Sequence[int], decode) -> List[Tuple[str, List[int]]]:
    """Pieces that decode to whole characters: an id whose bytes end inside a UTF-8 sequence decodes to U+FFFD and is carried over to
    the next id - unless the full text has a genuine U+FFFD at that place."""
    full = decode(list(ids))
    out: List[Tuple[str, List[int]]] = []
    cur: List[int] = []
    offset = 0
    for k, _ in enumerate(ids):
        cur.append(k)
        text = decode([ids[i] for i in cur])
        at = text.find("�")
        if at < 0 or (offset + at < len(full) and full[offset + at] == "�"):
            out.append((text, cur))
            cur = []
            offset += len(text)
    return out


def split_tokens_on_spaces(ids: Sequence[int], decode, eot: Optional[int] = None) -> List[Tuple[str, List[int]]]:
    """Words of a language written with spaces: a piece opens a word when it starts with a space, is punctuation, is a special id
    (>= ``eot``) or is the first; every other piece continues the word before it."""
    out: List[Tuple[str, List[int]]] = []
    for text, pos in split_tokens_on_unicode(ids, decode):
        special = eot is not None and ids[pos[0]] >= eot
        if special or text.startswith(" ") or text.strip() in _PUNCTUATION or not out:
            out.append((text, list(pos)))
        else:
            out[-1] = (out[-1][0] + text, out[-1][1] + list(pos))
    return out


def merge_punctuations(groups: List[Tuple[str, List[int]]], prepended: str = PREPEND_PUNCTUATIONS, appended: str = APPEND_PUNCTUATIONS) -> List[Tuple[str, List[int]]]:
    """Opening punctuation joins the word behind it, closing punctuation the word before it; the emptied groups are dropped."""
    g = [[t, list(p)] for t, p in groups]
    i, j = len(g) - 2, len(g) - 1
    while i >= 0:
        if g[i][0].startswith(" ") and g[i][0].strip() in prepended:
            g[j][0], g[j][1] = g[i][0] + g[j][0], g[i][1] + g[j][1]
            g[i][0], g[i][1] = "", []
        else:
            j = i
        i -= 1
    i, j = 0, 1
    while j < len(g):
        if not g[i][0].endswith(" ") and g[j][0] in appended:
            g[i][0], g[i][1] = g[i][0] + g[j][0], g[i][1] + g[j][1]
            g[j][0], g[j][1] = "", []
        else:
            i = j
        j += 1
    return [(t, p) for t, p in g if p]


def group_words(ids: Sequence[int], decode=None, eot: Optional[int] = None, spaces: bool = True) -> List[Tuple[str, List[int]]]:
    """The words of ``ids`` as (text, positions).  Without ``decode`` (a model without a tokenizer) every id is the word ``"<id>"``, as
    ``WhisperTranscriber._text`` renders them."""
    if decode is None:
        return [(f"<{int(t)}>", [k]) for k, t in enumerate(ids)]
    pieces = split_tokens_on_spaces(ids, decode, eot) if spaces else split_tokens_on_unicode(ids, decode)
    return merge_punctuations(pieces)


def words_from_times(ids: Sequence[int], times: "SttTokenTimes", first: int, groups: List[Tuple[str, List[int]]], shift: float = 0.0) -> List["SttWord"]:
    """``groups`` over ``ids`` - which are the ids ``first ..`` of the window ``times`` speaks of - as words: a word starts with its first
    id and ends with its last, and its probability is exp(mean log-probability)."""
    out = []
    for text, pos in groups:
        lp = [times.logprob[first + k] for k in pos]
        out.append(SttWord(text, shift + times.start[first + pos[0]], shift + times.end[first + pos[-1]], math.exp(sum(lp) / len(lp)), [int(ids[k]) for k in pos]))
    return out


MAX_ALIGNMENT_HEADS, MAX_MEDIAN_WIDTH = 32, 31       # rt_stt_set_alignment's limits


def alignment_error(cfg: "SttConfig") -> Optional[str]:
    """Why ``cfg``'s alignment heads and median width cannot be set on a model (rt_stt_set_alignment's rules, checked before anything
    touches a device), or None.  Word times are optional: a model they cannot be set on loads and transcribes as before, and
    ``NativeSTT.align_ids`` raises with this text."""
    heads, width = cfg.aligned_heads, cfg.median_filter_width
    where = "the configuration's alignment_heads" if cfg.alignment_heads is not None else \
        "the default (every head of the upper half of the decoder; give SttConfig.alignment_heads or a generation config's `alignment_heads`)"
    if not 1 <= len(heads) <= MAX_ALIGNMENT_HEADS:
        return f"{where} names {len(heads)} heads; word times take 1 .. {MAX_ALIGNMENT_HEADS}"
    if len(set(heads)) != len(heads) or any(not (0 <= l < cfg.dec_layers and 0 <= h < cfg.heads) for l, h in heads):
        return f"{where} holds a pair twice or outside {cfg.dec_layers} decoder layers of {cfg.heads} heads"
    if isinstance(width, bool) or not isinstance(width, (int, np.integer)) or not 1 <= int(width) <= MAX_MEDIAN_WIDTH or int(width) % 2 == 0:
        return f"median_filter_width must be an odd integer in 1 .. {MAX_MEDIAN_WIDTH}, got {width!r}"
    return None


class NativeSTT:
    """One ``rt_stt``: the speech-to-text model in HBM, on the context (GPU, stream) of the TTS engine it validates."""

    def __init__(self, ctx: "_native.Context", cfg: SttConfig, state: Dict[str, torch.Tensor]):
        self.ctx, self.cfg, self.lib = ctx, cfg, ctx.lib
        _declare(self.lib)
        self.rt_cfg = _rt_config(cfg)
        h = C.c_void_p()
        ctx.check(self.lib.rt_stt_create(ctx.handle, C.byref(self.rt_cfg), C.byref(h)), "rt_stt_create")
        self.handle = h
        native = to_native(state, cfg)
        n = self.lib.rt_stt_tensor_count(self.handle)
        for i in range(n):
            name = C.create_string_buffer(128)
            shp = (C.c_int64 * 2)()
            kind = C.c_int32()
            ctx.check(self.lib.rt_stt_tensor_info(self.handle, i, name, 128, shp, C.byref(kind)), "rt_stt_tensor_info")
            t = native.pop(name.value.decode()).contiguous()
            rows, cols = (t.shape[0], t.shape[1]) if t.dim() == 2 else (t.numel(), 1)
            if t.is_cuda:
                torch.cuda.current_stream(t.device).synchronize()
            ctx.check(self.lib.rt_stt_set_tensor(self.handle, name.value, C.c_void_p(t.data_ptr()), DT_BF16 if t.dtype == torch.bfloat16 else DT_F32,
                                                 rows, cols, 1 if t.is_cuda else 0), f"rt_stt_set_tensor({name.value.decode()})")
        if native:
            raise ValueError(f"tensors not consumed by the library: {sorted(native)[:4]}")
        if cfg.suppress_tokens:
            ids = (C.c_int32 * len(cfg.suppress_tokens))(*[int(t) for t in cfg.suppress_tokens])
            ctx.check(self.lib.rt_stt_set_suppress(self.handle, ids, len(cfg.suppress_tokens)), "rt_stt_set_suppress")
        if cfg.languages:
            lang = sorted(int(v) for v in cfg.languages.values())
            ctx.check(self.lib.rt_stt_set_languages(self.handle, (C.c_int32 * len(lang))(*lang), len(lang), int(cfg.no_speech_id)), "rt_stt_set_languages")
        if cfg.timestamp_begin is not None:
            ctx.check(self.lib.rt_stt_set_timestamps(self.handle, int(cfg.timestamp_begin), int(cfg.n_timestamps)), "rt_stt_set_timestamps")
        ctx.check(self.lib.rt_stt_finalize(self.handle), "rt_stt_finalize")
        self._set_alignment()

    def _set_alignment(self) -> None:
        """Word times are optional: heads that cannot be set (``alignment_error``) leave the model as it was before they existed - no
        native call, nothing raised - and ``align_ids`` raises at use."""
        cfg = self.cfg
        self.alignment_error = alignment_error(cfg)
        if self.alignment_error is None:
            heads = cfg.aligned_heads
            flat = (C.c_int32 * (2 * len(heads)))(*[int(v) for pair in heads for v in pair])
            if self.lib.rt_stt_set_alignment(self.handle, flat, len(heads), int(cfg.median_filter_width)) != _native.RT_OK:
                self.alignment_error = "rt_stt_set_alignment refused the alignment heads"

    def close(self) -> None:
        if getattr(self, "handle", None):
            self.lib.rt_stt_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass

    def _pcm(self, audio) -> torch.Tensor:
        x = audio if isinstance(audio, torch.Tensor) else torch.as_tensor(np.asarray(audio, dtype=np.float32))
        x = x.detach().reshape(-1).to(device=f"cuda:{self.ctx.device_ordinal}", dtype=torch.float32).contiguous()
        torch.cuda.current_stream(x.device).synchronize()
        return x

    def transcribe_ids(self, audio, sample_rate: int, max_tokens: Optional[int] = None, first_logits: bool = False):
        x = self._pcm(audio)
        # audio longer than one chunk is transcribed window by window (rt_stt_transcribe): room for every window's ids
        cap = int(max_tokens or self.windows(x.numel(), sample_rate) * self.cfg.max_new_tokens)
        toks = (C.c_int32 * cap)()
        n = C.c_int32()
        lg = torch.empty(self.cfg.vocab, dtype=torch.float32, device=x.device) if first_logits else None
        self.ctx.check(self.lib.rt_stt_transcribe(self.handle, C.c_void_p(x.data_ptr() if x.numel() else 0), x.numel(), int(sample_rate), toks, cap,
                                                  C.byref(n), C.c_void_p(lg.data_ptr()) if lg is not None else None), "rt_stt_transcribe")
        ids = [int(toks[i]) for i in range(n.value)]
        return (ids, lg) if first_logits else ids

    def windows(self, n_samples: int, sample_rate: int) -> int:
        """``chunk_seconds`` windows a clip of ``n_samples`` is cut into (rt_stt_transcribe: an empty clip is one window of silence)."""
        return max(1, -(-int(n_samples) // (int(self.cfg.chunk_seconds) * int(sample_rate))))

    # What the batched methods share: the argument checks (before anything touches a device), the clips as pointer and length
    # arrays, room for every window's ids, the languages as an array
    def _check(self, who: str, beam_size, max_tokens) -> None:
        check_beam_size(beam_size)
        if max_tokens is not None and int(max_tokens) < 1:
            raise ValueError(f"max_tokens must be at least 1, got {max_tokens!r}")
        if not getattr(self, "handle", None):
            raise ValueError(f"{who}: the model is closed")

    def _clips(self, audios):
        xs = [self._pcm(a) for a in audios]
        n = len(xs)
        ptrs = (C.c_void_p * max(n, 1))(*[x.data_ptr() if x.numel() else None for x in xs])
        lens = (C.c_int64 * max(n, 1))(*[x.numel() for x in xs])
        return xs, n, ptrs, lens

    def _token_cap(self, n_win: Sequence[int], max_tokens: Optional[int]) -> int:
        """``max_tokens``, or room for every window (``n_win``: per clip) of the longest clip, so nothing is cut."""
        return int(max_tokens or max(list(n_win) or [1]) * self.cfg.max_new_tokens)

    def _languages(self, languages, n: int):
        """``languages`` of a call over ``n`` clips (one entry for all or one per clip) as rt_stt_decode_opts.h_language; None stays None."""
        if languages is None:
            return None
        each = [languages] * n if isinstance(languages, (str, int, np.integer)) else list(languages)
        if len(each) != n:
            raise ValueError(f"{len(each)} languages for {n} clips")
        return (C.c_int32 * max(n, 1))(*[self._language_id(v) for v in each])

    def transcribe_ids_batch(self, audios, sample_rate: int, max_tokens: Optional[int] = None) -> List[List[int]]:
        """The ids of every clip from ONE native call (rt_stt_transcribe_batch): per clip what ``transcribe_ids`` gives for it alone.
        ``max_tokens`` caps every clip; the default leaves room for every window of the longest clip, so nothing is cut."""
        xs, n, ptrs, lens = self._clips(audios)
        cap = self._token_cap([self.windows(x.numel(), sample_rate) for x in xs], max_tokens)
        toks, counts = _i32(n * cap), _i32(n)
        self.ctx.check(self.lib.rt_stt_transcribe_batch(self.handle, ptrs, lens, n, int(sample_rate), toks, cap, counts), "rt_stt_transcribe_batch")
        return _clip_ids(toks, counts, n, cap)

    def transcribe_ids_beam(self, audios, sample_rate: int, beam_size: int, max_tokens: Optional[int] = None) -> Tuple[List[List[int]], List[float]]:
        """Beam search of width ``beam_size`` (1 .. 8) over every clip from ONE native call (rt_stt_transcribe_beam): the ids, and per
        clip the average log-probability per emitted token (end-of-sequence counted) of the chosen hypotheses.  A clip's ids and score
        are what it gets alone; ``beam_size == 1`` gives the ids of ``transcribe_ids_batch``.  ``max_tokens`` caps every clip's ids."""
        self._check("transcribe_ids_beam", beam_size, max_tokens)
        xs, n, ptrs, lens = self._clips(audios)
        cap = self._token_cap([self.windows(x.numel(), sample_rate) for x in xs], max_tokens)
        toks, counts, scores = _i32(n * cap), _i32(n), _f32(n)
        self.ctx.check(self.lib.rt_stt_transcribe_beam(self.handle, ptrs, lens, n, int(sample_rate), int(beam_size), toks, cap, counts, scores),
                       "rt_stt_transcribe_beam")
        return _clip_ids(toks, counts, n, cap), [float(scores[i]) for i in range(n)]

    def _language_id(self, language) -> int:
        """A code ("zh"), "auto" / None (-1: detect) or a token id, as an entry of rt_stt_decode_opts.h_language."""
        if language is None or language == "auto":
            return -1
        if isinstance(language, str):
            if language not in self.cfg.languages:
                raise ValueError(f"unknown language {language!r}: the model knows {sorted(self.cfg.languages)}")
            return int(self.cfg.languages[language])
        return int(language)

    def detect_language(self, audios, sample_rate: int) -> List[Tuple[int, float, float]]:
        """Per clip (language id, its probability among the configured ids, no-speech probability), decided on the clip's first
        window (rt_stt_detect_language; the rule: DESIGN.md section 5).  ``cfg.language_code`` gives the code of an id."""
        if not getattr(self, "handle", None):
            raise ValueError("detect_language: the model is closed")
        xs, n, ptrs, lens = self._clips(audios)
        lang, prob, ns = (C.c_int32 * max(n, 1))(), (C.c_float * max(n, 1))(), (C.c_float * max(n, 1))()
        self.ctx.check(self.lib.rt_stt_detect_language(self.handle, ptrs, lens, n, int(sample_rate), lang, prob, ns), "rt_stt_detect_language")
        return [(int(lang[i]), float(prob[i]), float(ns[i])) for i in range(n)]

    def transcribe_ids_ex(self, audios, sample_rate: int, beam_size: int = 1, languages=None, max_tokens: Optional[int] = None,
                          no_speech: bool = True) -> List[SttClip]:
        """``transcribe_ids_beam`` with a language per clip and a report per window, from ONE native call (rt_stt_transcribe_ex).
        ``languages``: None - the configured prefix; one entry for all clips or one per clip: a code, a token id, or "auto" / None /
        -1 to detect the clip's language on its first window.  ``no_speech``: ask for the windows' no-speech probabilities (the
        probe pass then runs even when every language is given)."""
        self._check("transcribe_ids_ex", beam_size, max_tokens)
        xs, n, ptrs, lens = self._clips(audios)
        n_win = [self.windows(x.numel(), sample_rate) for x in xs]
        cap, wcap = self._token_cap(n_win, max_tokens), sum(n_win)
        opts, out = RtSttDecodeOpts(), RtSttDecodeOut()
        opts.beam_size, opts.max_tokens = int(beam_size), cap
        req = self._languages(languages, n)
        if req is not None:
            opts.h_language = req
        toks, counts, scores, lang, lprob = _i32(n * cap), _i32(n), _f32(n), _i32(n), _f32(n)
        w_clip, w_n, w_lp, w_ns = _i32(wcap), _i32(wcap), _f32(wcap), _f32(wcap)
        out.h_tokens, out.h_n_tokens, out.h_scores, out.h_language, out.h_language_prob = toks, counts, scores, lang, lprob
        out.h_win_clip, out.h_win_n_ids, out.h_win_logprob, out.window_cap = w_clip, w_n, w_lp, wcap
        if no_speech:
            out.h_win_no_speech = w_ns
        self.ctx.check(self.lib.rt_stt_transcribe_ex(self.handle, ptrs, lens, n, int(sample_rate), C.byref(opts), C.byref(out)), "rt_stt_transcribe_ex")
        clips = [SttClip(ids, float(scores[i]), int(lang[i]), float(lprob[i]), []) for i, ids in enumerate(_clip_ids(toks, counts, n, cap))]
        for w in range(out.n_windows):
            clips[w_clip[w]].windows.append(SttWindow(int(w_n[w]), float(w_lp[w]), float(w_ns[w]) if no_speech else float("nan")))
        return clips

    @property
    def align_room(self) -> int:
        """The text ids one window of ``align_ids`` takes: the text context behind the forced prefix, less the end-of-sequence row."""
        return int(self.cfg.n_text_ctx) - len(self.cfg.prefix) - 1

    def align_ids(self, windows, sample_rate: int, ids, languages=None) -> List[SttTokenTimes]:
        """Forced alignment of known text from ONE native call (rt_stt_align; the rule: DESIGN.md section 5, "word times"): every entry
        of ``windows`` is one window of at most ``chunk_seconds`` and ``ids[w]`` its text ids (no timestamp ids, no end-of-sequence, at
        most ``align_room``).  Per window the start and end of every id in seconds of the window and its log-probability.
        ``languages``: None - the configured prefix; else a code or token id for all windows or one per window (no detection)."""
        if not getattr(self, "handle", None):
            raise ValueError("align_ids: the model is closed")
        if getattr(self, "alignment_error", None):
            raise ValueError(f"align_ids: this model has no alignment heads: {self.alignment_error}")
        ids = [[int(t) for t in w] for w in ids]
        xs, n, ptrs, lens = self._clips(windows)
        if len(ids) != n:
            raise ValueError(f"{len(ids)} id lists for {n} windows")
        limit = int(self.cfg.chunk_seconds) * int(sample_rate)
        for w, (x, t) in enumerate(zip(xs, ids)):
            if x.numel() > limit:
                raise ValueError(f"align_ids: window {w} has {x.numel()} samples; one window is at most {self.cfg.chunk_seconds} s ({limit} samples)")
            if len(t) > self.align_room:
                raise ValueError(f"align_ids: window {w} has {len(t)} text ids; one window takes at most {self.align_room}")
            if any(not 0 <= v < self.cfg.eos_id for v in t):
                raise ValueError(f"align_ids: window {w} holds an id outside the text ids [0, {self.cfg.eos_id}): no special or timestamp ids")
        req = self._languages(languages, n)
        if req is not None and any(v < 0 for v in req):
            raise ValueError("align_ids: a window's language must be given (no detection here: use detect_language)")
        offs = [0]
        for t in ids:
            offs.append(offs[-1] + len(t))
        n_rows = sum(len(t) + 1 for t in ids if t)
        flat = (C.c_int32 * max(offs[-1], 1))(*[t for w in ids for t in w])
        frames, lps, nfr = _i32(n_rows), _f32(offs[-1]), _i32(n)
        out = RtSttAlignOut()
        out.h_token_frame, out.h_token_logprob, out.h_n_frames = frames, lps, nfr
        self.ctx.check(self.lib.rt_stt_align(self.handle, ptrs, lens, n, int(sample_rate), flat, (C.c_int32 * (n + 1))(*offs), req, C.byref(out)), "rt_stt_align")
        res, at = [], 0
        for w, t in enumerate(ids):
            k = len(t)
            fr = [int(frames[at + i]) for i in range(k + 1)] if k else []
            at += k + 1 if k else 0
            res.append(SttTokenTimes([f * FRAME_SECONDS for f in fr[:-1]], [f * FRAME_SECONDS for f in fr[1:]], [float(lps[offs[w] + i]) for i in range(k)], int(nfr[w])))
        return res

    def seek_caps(self, n_samples: Sequence[int], sample_rate: int) -> Tuple[int, int, int]:
        """(tokens per clip, segments, windows) the first attempt of ``transcribe_ids_seek`` leaves room for.  A repeat costs a whole
        decode and room costs a few integers, so the guess is generous: per clip twice its fixed-cut windows plus two, and per
        window the most segments its tokens can close (a segment takes a text id and a timestamp at least).  The call reports what
        it needed when that is short."""
        n_win = [2 * self.windows(n, sample_rate) + 2 for n in n_samples]
        per_window = int(self.cfg.max_new_tokens) // 2 + 1
        return max(n_win or [1]) * int(self.cfg.max_new_tokens), max(1, sum(n_win) * per_window), max(1, sum(n_win))

    def transcribe_ids_seek(self, audios, sample_rate: int, beam_size: int = 1, languages=None, max_tokens: Optional[int] = None,
                            max_initial_timestamp_index: Optional[int] = None, no_speech_threshold: Optional[float] = None,
                            logprob_threshold: Optional[float] = -1.0, no_speech: bool = True, caps: Optional[Tuple[int, int, int]] = None) -> List[SttSeekClip]:
        """Clips of any length by timestamps and seek (rt_stt_transcribe_seek; the rules: DESIGN.md section 5): per clip the text ids of
        its closed segments, the segments with their times and the windows the call decoded.  ``languages`` as ``transcribe_ids_ex``;
        ``max_initial_timestamp_index`` None: the configuration's (-1: no limit); ``no_speech_threshold`` not None switches the silence
        rule on (validation.window_is_silent): a silent window gives no segment and is consumed whole.  ``caps``: room for (tokens per
        clip, segments, windows) at the first attempt (default: ``seek_caps``); when one runs out the call is repeated ONCE with the
        counts the library reported, so a result is never cut - except the ids at an explicit ``max_tokens``."""
        self._check("transcribe_ids_seek", beam_size, max_tokens)
        if self.cfg.timestamp_begin is None:
            raise ValueError("transcribe_ids_seek: the configuration has no timestamp ids (SttConfig.timestamp_begin)")
        xs, n, ptrs, lens = self._clips(audios)
        tcap, scap, wcap = caps or self.seek_caps([x.numel() for x in xs], sample_rate)
        if max_tokens is not None:
            tcap = int(max_tokens)
        req = self._languages(languages, n)
        mi = self.cfg.max_initial_timestamp_index if max_initial_timestamp_index is None else int(max_initial_timestamp_index)
        nan = float("nan")
        for attempt in range(2):
            opts, out = RtSttSeekOpts(), RtSttSeekOut()
            opts.beam_size, opts.max_tokens, opts.max_initial_timestamp_index = int(beam_size), int(tcap), int(mi)
            opts.no_speech_threshold = nan if no_speech_threshold is None else float(no_speech_threshold)
            opts.logprob_threshold = nan if logprob_threshold is None else float(logprob_threshold)
            if req is not None:
                opts.h_language = req
            toks, counts, scores, lang, lprob = _i32(n * tcap), _i32(n), _f32(n), _i32(n), _f32(n)
            g_clip, g_s, g_e, g_st, g_et, g_n = _i32(scap), _f32(scap), _f32(scap), _i32(scap), _i32(scap), _i32(scap)
            w_clip, w_off, w_n, w_lp, w_ns, w_adv = _i32(wcap), (C.c_int64 * max(wcap, 1))(), _i32(wcap), _f32(wcap), _f32(wcap), _i32(wcap)
            out.h_tokens, out.h_n_tokens, out.h_scores, out.h_language, out.h_language_prob = toks, counts, scores, lang, lprob
            out.h_seg_clip, out.h_seg_start, out.h_seg_end, out.h_seg_start_tick, out.h_seg_end_tick, out.h_seg_n_ids = g_clip, g_s, g_e, g_st, g_et, g_n
            out.h_win_clip, out.h_win_offset, out.h_win_n_ids, out.h_win_logprob, out.h_win_advance = w_clip, w_off, w_n, w_lp, w_adv
            if no_speech or no_speech_threshold is not None:
                out.h_win_no_speech = w_ns
            out.segment_cap, out.window_cap = int(scap), int(wcap)
            rc = self.lib.rt_stt_transcribe_seek(self.handle, ptrs, lens, n, int(sample_rate), C.byref(opts), C.byref(out))
            short = out.n_segments > scap or out.n_windows > wcap or (max_tokens is None and out.max_clip_tokens > tcap)
            if rc not in (_native.RT_OK, _native.RT_ERR_LENGTH) or not short:
                self.ctx.check(rc, "rt_stt_transcribe_seek")
                break
            if attempt == 1:
                raise RuntimeError(f"rt_stt_transcribe_seek: length: the repeated call needed {out.n_segments} segments, {out.n_windows} windows and "
                                   f"{out.max_clip_tokens} ids, not the {scap}, {wcap} and {tcap} it reported before")
            scap, wcap = max(scap, out.n_segments), max(wcap, out.n_windows)
            if max_tokens is None:
                tcap = max(tcap, out.max_clip_tokens)
        clips = [SttSeekClip(ids, float(scores[i]), int(lang[i]), float(lprob[i]), [], []) for i, ids in enumerate(_clip_ids(toks, counts, n, tcap))]
        at = [0] * n
        for g in range(out.n_segments):
            i = g_clip[g]
            ids = clips[i].ids[at[i]:at[i] + g_n[g]]                  # (an explicit max_tokens leaves the last segments short)
            at[i] += g_n[g]
            clips[i].segments.append(SttSegment(float(g_s[g]), float(g_e[g]), ids, int(g_st[g]), int(g_et[g])))
        for w in range(out.n_windows):
            clips[w_clip[w]].windows.append(SttSeekWindow(int(w_off[w]), int(w_n[w]), float(w_lp[w]), float(w_ns[w]) if out.h_win_no_speech else nan, int(w_adv[w])))
        if self._prompt_set:                                      # the report's lines follow the per-window arrays: clip by clip
            lines = iter(self.prompt_report())
            for c in clips:
                c.windows = [dataclasses.replace(w, prompt_len=next(lines).prompt_len) for w in c.windows]
        return clips

    _prompt_set = False

    def set_prompt(self, initial_ids=None, condition_on_previous: bool = False, reset_on_temperature: Optional[float] = 0.5) -> None:
        """Conditioning on previous text and an initial prompt for ``transcribe_ids_seek`` (rt_stt_set_prompt; the rule: DESIGN.md
        section 5, "conditioning on previous text", restated in validation.prompt_for_window / history_after_window).
        ``initial_ids``: token ids in front of every clip's first window; ``condition_on_previous``: every later window decodes behind
        the tail of what its clip produced so far; ``reset_on_temperature``: that history is dropped behind a window whose chosen
        attempt ran above this temperature (None: never).  Neither ``initial_ids`` nor ``condition_on_previous``: the policy is
        cleared, and every call is what it is without one."""
        if not getattr(self, "handle", None):
            raise ValueError("set_prompt: the model is closed")
        if not initial_ids and not condition_on_previous:
            self.ctx.check(self.lib.rt_stt_set_prompt(self.handle, None), "rt_stt_set_prompt")
            self._prompt_set = False
            return
        ids, reset = check_prompt_args(self.cfg, initial_ids, condition_on_previous, reset_on_temperature)
        p = RtSttPrompt()
        p.sot_prev_id, p.condition_on_previous, p.reset_on_temperature = int(self.cfg.sot_prev_id), 1 if condition_on_previous else 0, float("nan") if reset is None else reset
        arr = (C.c_int32 * max(len(ids), 1))(*ids)
        if ids:
            p.h_initial, p.n_initial = arr, len(ids)
        self.ctx.check(self.lib.rt_stt_set_prompt(self.handle, C.byref(p)), "rt_stt_set_prompt")
        self._prompt_set = True

    def prompt_report(self) -> List[SttPromptWindow]:
        """Per window of the last ``transcribe_ids_seek`` call under a prompt policy, in the order of that call's windows (clip by clip)."""
        n = C.c_int32()
        rc = self.lib.rt_stt_prompt_report(self.handle, 0, None, None, C.byref(n))
        if rc not in (_native.RT_OK, _native.RT_ERR_LENGTH):
            self.ctx.check(rc, "rt_stt_prompt_report")
        k = n.value
        ln, rs = _i32(k), _i32(k)
        self.ctx.check(self.lib.rt_stt_prompt_report(self.handle, k, ln, rs, C.byref(n)), "rt_stt_prompt_report")
        return [SttPromptWindow(int(ln[i]), bool(rs[i])) for i in range(n.value)]

    def set_fallback(self, temperatures, best_of: int = 5, compression_ratio_threshold: Optional[float] = 2.4, logprob_threshold: Optional[float] = -1.0,
                     no_speech_threshold: Optional[float] = None, seed: int = 789, ratio=None) -> None:
        """The temperature fallback of ``transcribe_ids_ex`` and ``transcribe_ids_seek`` (rt_stt_set_fallback; the rule: DESIGN.md section
        5, "temperature fallback", restated in validation.needs_fallback / pick_attempt): a window whose attempt compresses above
        ``compression_ratio_threshold`` or averages below ``logprob_threshold`` is decoded again at the next of ``temperatures`` - 0:
        the beam decode of the call's width; above 0: ``best_of`` sampled rows - over the encoder states the call still holds.
        ``temperatures`` None clears the policy.  ``ratio``: a callable on the list of an attempt's text ids (default, with a
        compression threshold: validation.compression_ratio_ids at the model's vocabulary; given without a threshold it decides
        nothing and only fills the report).  It runs inside the
        native call, on the calling thread, with the context locked: it must not call into this model or its context.  A threshold
        of None is off; ``no_speech_threshold`` exempts silent windows (it needs a model with languages)."""
        if not getattr(self, "handle", None):
            raise ValueError("set_fallback: the model is closed")
        if temperatures is None:
            self.ctx.check(self.lib.rt_stt_set_fallback(self.handle, None), "rt_stt_set_fallback")
            self._ratio_cb = None
            return
        ts = check_temperatures(temperatures)
        if isinstance(best_of, bool) or not isinstance(best_of, (int, np.integer)) or not 1 <= int(best_of) <= MAX_BEAM:
            raise ValueError(f"best_of must be an integer in 1 .. {MAX_BEAM}, got {best_of!r}")
        nan = float("nan")
        f = RtSttFallback()
        f.n_temperatures, f.best_of, f.seed = len(ts), int(best_of), int(seed) & 0xFFFFFFFFFFFFFFFF
        for i, t in enumerate(ts):
            f.temperatures[i] = t
        f.compression_ratio_threshold = nan if compression_ratio_threshold is None else float(compression_ratio_threshold)
        f.logprob_threshold = nan if logprob_threshold is None else float(logprob_threshold)
        f.no_speech_threshold = nan if no_speech_threshold is None else float(no_speech_threshold)
        cb = None
        if compression_ratio_threshold is not None or ratio is not None:     # (a callback without a threshold only fills the report)
            if ratio is None:
                from .validation import compression_ratio_ids
                vocab = int(self.cfg.vocab)
                ratio = lambda ids: compression_ratio_ids(ids, vocab)          # noqa: E731
            if isinstance(ratio, RATIO_FN):
                cb = ratio
            else:
                fn = ratio

                def _ratio(p_ids, n, _user):
                    try:
                        return float(fn([int(p_ids[i]) for i in range(n)]))
                    except Exception:  # noqa: BLE001  (nothing may unwind through the native frames: NaN fails the call there)
                        return float("nan")
                cb = RATIO_FN(_ratio)
            f.ratio = cb
        self.ctx.check(self.lib.rt_stt_set_fallback(self.handle, C.byref(f)), "rt_stt_set_fallback")
        self._ratio_cb = cb                                          # (the library calls it for as long as the policy stands)

    def fallback_report(self) -> List[SttFallbackWindow]:
        """Per window of the last ``transcribe_ids_ex`` / ``transcribe_ids_seek`` call under a policy, in the order of that call's windows
        (clip by clip): attempts, the chosen attempt's temperature and compression ratio."""
        n = C.c_int32()
        rc = self.lib.rt_stt_fallback_report(self.handle, 0, None, None, None, C.byref(n))
        if rc not in (_native.RT_OK, _native.RT_ERR_LENGTH):
            self.ctx.check(rc, "rt_stt_fallback_report")
        k = n.value
        att, tmp, rat = _i32(k), _f32(k), _f32(k)
        self.ctx.check(self.lib.rt_stt_fallback_report(self.handle, k, att, tmp, rat, C.byref(n)), "rt_stt_fallback_report")
        return [SttFallbackWindow(int(att[i]), float(tmp[i]), float(rat[i])) for i in range(n.value)]

    def log_mel(self, audio, sample_rate: int) -> torch.Tensor:
        """[n_mels][frames] float32 (the layout of WhisperFeatureExtractor's ``input_features``)."""
        x = self._pcm(audio)
        out = torch.empty(2 * self.cfg.n_ctx, self.cfg.n_mels, dtype=torch.float32, device=x.device)
        self.ctx.check(self.lib.rt_stt_log_mel(self.handle, C.c_void_p(x.data_ptr() if x.numel() else 0), x.numel(), int(sample_rate),
                                               C.c_void_p(out.data_ptr())), "rt_stt_log_mel")
        return out.t().contiguous()

    def encode(self, audio, sample_rate: int) -> torch.Tensor:
        x = self._pcm(audio)
        out = torch.empty(self.cfg.n_ctx, self.cfg.d_model, dtype=torch.float32, device=x.device)
        self.ctx.check(self.lib.rt_stt_encode(self.handle, C.c_void_p(x.data_ptr() if x.numel() else 0), x.numel(), int(sample_rate),
                                              C.c_void_p(out.data_ptr())), "rt_stt_encode")
        return out


def join_segment_texts(texts) -> str:
    """A clip's text from its segments' texts, as the reference joins them: ``" ".join(segment.text ...)`` and a final strip
    (stt_validator.py:136, :143)."""
    return " ".join(texts).strip()


def check_timestamp_config(cfg: SttConfig, timestamps: bool) -> None:
    """``WhisperTranscriber(timestamps=True)`` needs a configuration with timestamp ids whose prefix ends in <|notimestamps|>."""
    if not timestamps:
        return
    tb = cfg.timestamp_begin
    if tb is None:
        raise ValueError("timestamps=True needs a model with timestamp ids (SttConfig.timestamp_begin)")
    if not cfg.prefix or cfg.prefix[-1] != tb - 1 or tb + cfg.n_timestamps > cfg.vocab:
        raise ValueError(f"timestamps=True: the prefix {tuple(cfg.prefix)} must end in <|notimestamps|> = {tb - 1} and the vocabulary of {cfg.vocab} "
                         f"hold the {cfg.n_timestamps} timestamp ids from {tb} on")


@dataclass
class SttDetail:
    """One clip of ``WhisperTranscriber.batch_detailed``.  (The defaults stand where a native call reports less: the greedy calls give
    ids alone, the plain beam call ids and a score - ``WhisperTranscriber._run``; ``batch_detailed`` fills every field.)"""
    text: Optional[str]
    ids: List[int]
    avg_logprob: float = float("nan")    # over the windows kept (over all of them when none is)
    language: Optional[str] = None       # the code at position 1 of the clip's prefix
    language_prob: float = float("nan")  # its probability where it was detected, 1 where it was given
    no_speech_prob: float = float("nan")  # the largest of the clip's windows
    windows_dropped: int = 0             # windows the silence rule left out
    # under a fallback policy (WhisperTranscriber(temperatures=...)), per window of the clip; empty without one
    temperature: List[float] = field(default_factory=list)
    attempts: List[int] = field(default_factory=list)
    compression_ratio: List[float] = field(default_factory=list)
    prompt_len: List[int] = field(default_factory=list)      # under a prompt policy, per window of the clip; empty without one


class WhisperTranscriber:
    """``transcriber`` hook of the provider: ``(audio tensor, sample_rate) -> text`` (None = transcription failed), the
    tensor-level stand-in for ``transcribe_audio(path)`` (stt_validator.py:116-148).  ``model_dir``: a local Whisper checkpoint
    (safetensors + config.json + tokenizer.json); without one the model runs on seeded synthetic weights - only when that is asked
    for explicitly - and the "text" is the generated ids written out, which is all random weights can mean.  ``beam_size``: 1
    decodes greedily (the single-clip and the batched call); a larger width sends every call through beam search
    (``transcribe_ids_beam``; faster-whisper, which the reference transcribes with, defaults to 5), and ``batch_scored`` returns
    each text with its confidence.  ``language``: the Whisper code the voice speaks ("en", "zh", ...; ``whisper_language`` maps the
    provider's names) - it takes position 1 of the forced prefix - or "auto": every clip's language is detected on its first window
    (``transcribe_ids_ex``).  ``no_speech_threshold`` (None: off; Whisper's transcribers use 0.6) and ``logprob_threshold`` switch the
    silence rule on (validation.window_is_silent): ``__call__`` and ``batch`` then go through ``transcribe_ids_ex`` and leave out the
    ids of silent windows, so that a silent clip is "" and not what the decoder makes up.  ``temperatures``: the temperature fallback
    (``NativeSTT.set_fallback``) - the default ``(0.0,)`` sets no policy; ``(0.0, 0.2, 0.4, 0.6, 0.8, 1.0)`` with ``best_of`` 5 and
    ``compression_ratio_threshold`` 2.4 is what the reference's ``model.transcribe`` runs with; the ratio is
    validation.compression_ratio_text of the attempt's text.  Calls then go through ``transcribe_ids_ex`` (or the seek call), and
    ``batch_detailed`` / ``batch_segments`` report ``temperature``, ``attempts`` and ``compression_ratio`` per window."""
    auto, no_speech_threshold, logprob_threshold = False, None, -1.0
    _ex = False                          # calls go through transcribe_ids_ex (a detected language, or the silence rule)
    timestamps = False                   # calls go through transcribe_ids_seek (the reference's long-form rule; see below)
    fallback = False                     # a fallback policy is set on the model (temperatures other than (0.0,))
    prompted = False                     # a prompt policy is set on the model (condition_on_previous_text / initial_prompt)
    word_timestamps = False              # batch_segments fills every segment's words (NativeSTT.align_ids)

    def __init__(self, ctx: "_native.Context", model_dir: Optional[str] = None, synthetic: bool = False, cfg: Optional[SttConfig] = None, seed: int = 789,
                 beam_size: int = 1, language: str = "en", no_speech_threshold: Optional[float] = None, logprob_threshold: Optional[float] = -1.0,
                 timestamps: bool = False, temperatures=(0.0,), best_of: int = 5, compression_ratio_threshold: Optional[float] = 2.4,
                 condition_on_previous_text: bool = False, initial_prompt=None, prompt_reset_on_temperature: Optional[float] = 0.5,
                 word_timestamps: bool = False):
        """``timestamps``: every call decodes with timestamp tokens and walks a clip longer than one window by seek positions
        (``transcribe_ids_seek``), as the reference's ``model.transcribe`` does; a clip's text is its segments' texts joined with a
        space (stt_validator.py:136), and ``batch_segments`` returns them with their times.  ``condition_on_previous_text``,
        ``initial_prompt`` and ``prompt_reset_on_temperature`` (``NativeSTT.set_prompt``; faster-whisper's options of the same names,
        which default to True, None and 0.5 there): both need ``timestamps=True``.  ``initial_prompt`` is a string - encoded as
        faster-whisper encodes it, ``" " + text.strip()`` through the tokenizer - or a sequence of token ids, the only form a model
        without a tokenizer takes.  ``batch_detailed`` / ``batch_segments`` then report ``prompt_len`` per window.
        ``word_timestamps`` (faster-whisper's option of the same name; needs ``timestamps=True``): ``batch_segments`` fills every
        segment's ``words`` from one more native call (``NativeSTT.align_ids``) over the windows the segments lie in."""
        if word_timestamps and not timestamps:
            raise ValueError("word_timestamps needs timestamps=True: words are placed inside the segments of the seek path")
        if (condition_on_previous_text or initial_prompt is not None) and not timestamps:
            raise ValueError("condition_on_previous_text and initial_prompt need timestamps=True: only the seek path has a previous window")
        self.beam_size = check_beam_size(beam_size)
        self.auto = language == "auto"
        self.no_speech_threshold, self.logprob_threshold = no_speech_threshold, logprob_threshold
        code = "en" if self.auto else language
        self.tokenizer = None
        dev = f"cuda:{ctx.device_ordinal}"
        if model_dir and os.path.isdir(model_dir) and any(f.endswith(".safetensors") for f in os.listdir(model_dir)):
            if cfg is None:
                cfg = SttConfig.from_dir(model_dir, code) if os.path.exists(os.path.join(model_dir, "config.json")) else SttConfig()
            state = load_checkpoint(cfg, model_dir, device=dev)
            tok_path = os.path.join(model_dir, "tokenizer.json")
            if os.path.exists(tok_path):
                from tokenizers import Tokenizer
                self.tokenizer = Tokenizer.from_file(tok_path)
        elif synthetic:
            cfg = cfg or SttConfig()
            state = synthetic_state(cfg, seed, device=dev)
        else:
            raise ValueError(f"no local Whisper checkpoint at {model_dir!r} (this build cannot download one); pass synthetic=True for seeded "
                             "random weights of the architecture (parity tests, benchmarks)")
        if code != cfg.language:
            cfg = cfg.with_language(code)
        if (self.auto or no_speech_threshold is not None) and not cfg.languages:
            raise ValueError("language detection and the silence rule need a model with language ids (SttConfig.languages)")
        self.timestamps = bool(timestamps)
        check_timestamp_config(cfg, self.timestamps)
        self.cfg = cfg
        temps = check_temperatures(temperatures)
        self.model = NativeSTT(ctx, cfg, state)
        self.word_timestamps = bool(word_timestamps)
        if self.word_timestamps and self.model.alignment_error:
            msg = self.model.alignment_error
            self.model.close()
            raise ValueError(f"word_timestamps=True: this model has no alignment heads: {msg}")
        self.fallback = temps != (0.0,)
        if self.fallback:
            from .validation import compression_ratio_text
            self.model.set_fallback(temps, best_of, compression_ratio_threshold, logprob_threshold, no_speech_threshold, seed,
                                    ratio=lambda ids: compression_ratio_text(self._text(ids) or ""))
        self._ex = self.auto or no_speech_threshold is not None or self.fallback       # calls that must go through transcribe_ids_ex
        self.prompted = False
        if condition_on_previous_text or initial_prompt is not None:
            try:
                self.model.set_prompt(self._prompt_ids(initial_prompt), bool(condition_on_previous_text), prompt_reset_on_temperature)
            except Exception:
                self.model.close()
                raise
            self.prompted = self.model._prompt_set               # (an empty prompt without conditioning sets no policy)

    def _prompt_ids(self, initial_prompt) -> Optional[List[int]]:
        if initial_prompt is None:
            return None
        if isinstance(initial_prompt, str):
            if self.tokenizer is None:
                raise ValueError("initial_prompt as a string needs a checkpoint with a tokenizer; pass token ids")
            return list(self.tokenizer.encode(" " + initial_prompt.strip(), add_special_tokens=False).ids)
        return list(initial_prompt)

    def _seek(self, audios, sample_rate: int) -> List[SttSeekClip]:
        return self.model.transcribe_ids_seek(audios, sample_rate, self.beam_size, "auto" if self.auto else None,
                                              no_speech_threshold=self.no_speech_threshold, logprob_threshold=self.logprob_threshold,
                                              no_speech=bool(self.cfg.languages))

    def _fallback_lines(self, clips) -> List[List[SttFallbackWindow]]:
        """``fallback_report`` of the call that returned ``clips``, cut per clip (no policy: empty lists)."""
        if not self.fallback:
            return [[] for _ in clips]
        lines, out, at = self.model.fallback_report(), [], 0
        for c in clips:
            out.append(lines[at:at + len(c.windows)])
            at += len(c.windows)
        return out

    @staticmethod
    def _fallback_fields(lines: List[SttFallbackWindow]) -> dict:
        return dict(temperature=[w.temperature for w in lines], attempts=[w.attempts for w in lines], compression_ratio=[w.compression_ratio for w in lines])

    def _segment_text(self, ids: List[int]) -> str:
        """One segment's text as the reference's transcriber hands it over (unstripped: the join and the final strip are the caller's)."""
        if self.tokenizer is not None:
            return self.tokenizer.decode(ids, skip_special_tokens=True)
        return " ".join(f"<{i}>" for i in ids)

    def _joined(self, clip: SttSeekClip) -> str:
        return join_segment_texts(self._segment_text(g.ids) for g in clip.segments)

    def batch_segments(self, audios, sample_rate: int) -> List[List[SttSegment]]:
        """Per clip its closed segments with start and end in seconds and their texts (``timestamps=True`` only)."""
        if not self.timestamps:
            raise ValueError("batch_segments needs WhisperTranscriber(timestamps=True)")
        clips = self._seek(audios, sample_rate)
        tick = int(0.02 * sample_rate)
        out = []
        for c, lines in zip(clips, self._fallback_lines(clips)):
            segs = []
            for g in c.segments:
                extra = {}
                if lines or self.prompted:                            # the window the segment lies in: the last one that starts at or before it
                    k = max(i for i, w in enumerate(c.windows) if w.offset // tick <= g.start_tick)
                    extra = dict(prompt_len=c.windows[k].prompt_len)
                    if lines:
                        extra.update(temperature=lines[k].temperature, attempts=lines[k].attempts, compression_ratio=lines[k].compression_ratio)
                segs.append(dataclasses.replace(g, text=self._segment_text(g.ids).strip(), **extra))
            out.append(segs)
        if self.word_timestamps:
            self._fill_words(list(audios), sample_rate, clips, out)
        return out

    def _decode_raw(self):
        """``decode(ids) -> str`` for the word grouping (ids rendered as they are), or None for a model without a tokenizer."""
        if self.tokenizer is None:
            return None
        return lambda ids: self.tokenizer.decode(list(ids), skip_special_tokens=False)

    def _words(self, ids: List[int], times: SttTokenTimes, first: int, shift: float, language: Optional[str] = None) -> List[SttWord]:
        spaces = (language or self.cfg.language) not in UNSPACED_LANGUAGES
        return words_from_times(ids, times, first, group_words(ids, self._decode_raw(), self.cfg.eos_id, spaces), shift)

    def _fill_words(self, audios, sample_rate: int, clips: List[SttSeekClip], out: List[List[SttSegment]]) -> None:
        """``words`` of every segment of ``out`` (``batch_segments``): segments are grouped by the window they lie in - the last window that
        starts at or before them - and every such window of every clip goes through ONE ``align_ids`` call with the segments' ids joined;
        times are shifted by the window's offset.  Under ``language="auto"`` a clip's windows are aligned, and split into words, under
        the language the seek call detected for the clip.  The text ids of one window fit ``align_room`` - a segment spends two of the
        window's at most ``n_text_ctx - n_prefix`` generated ids on its timestamps - so a window that holds more is an error."""
        tick, win, room = int(0.02 * sample_rate), int(self.cfg.chunk_seconds) * int(sample_rate), self.model.align_room
        jobs = []                                                     # (audio, offset in samples, [segments], the clip's language id)
        for audio, c, segs in zip(audios, clips, out):
            x = audio if isinstance(audio, torch.Tensor) else torch.as_tensor(np.asarray(audio, dtype=np.float32))
            x = x.detach().reshape(-1)
            by_window: Dict[int, List[SttSegment]] = {}
            for g in segs:
                g.words = []
                if g.ids:
                    k = max(i for i, w in enumerate(c.windows) if w.offset // tick <= g.start_tick)
                    by_window.setdefault(k, []).append(g)
            for k in sorted(by_window):
                n = sum(len(g.ids) for g in by_window[k])
                if n > room:
                    raise RuntimeError(f"word_timestamps: the segments of the window at sample {c.windows[k].offset} hold {n} text ids; one window takes {room}")
                jobs.append((x, c.windows[k].offset, by_window[k], int(c.language)))
        if not jobs:
            return
        times = self.model.align_ids([x[off:off + win] for x, off, _, _ in jobs], sample_rate, [[t for g in piece for t in g.ids] for _, _, piece, _ in jobs],
                                     languages=[lang for _, _, _, lang in jobs] if self.auto else None)
        for (x, off, piece, lang), tt in zip(jobs, times):
            first = 0
            for g in piece:
                g.words = self._words(g.ids, tt, first, off / float(sample_rate), self.cfg.language_code(lang) if self.auto else None)
                first += len(g.ids)

    def align(self, audios, sample_rate: int, texts_or_ids) -> List[List[SttWord]]:
        """Forced alignment of known text to audio, one window per clip: per clip the words of its text with their times in seconds of
        the clip.  ``texts_or_ids``: per clip a string - encoded as ``initial_prompt`` is, ``" " + text.strip()`` through the tokenizer,
        which a model without one cannot do - or a sequence of token ids.  A clip longer than one window raises."""
        audios, texts_or_ids = list(audios), list(texts_or_ids)
        if len(audios) != len(texts_or_ids):
            raise ValueError(f"{len(texts_or_ids)} texts for {len(audios)} clips")
        limit = int(self.cfg.chunk_seconds) * int(sample_rate)
        ids = []
        for i, (a, t) in enumerate(zip(audios, texts_or_ids)):
            n = a.numel() if isinstance(a, torch.Tensor) else int(np.asarray(a).size)
            if n > limit:
                raise ValueError(f"align: clip {i} has {n} samples; forced alignment takes one window of at most {self.cfg.chunk_seconds} s ({limit} samples) per clip")
            if isinstance(t, str):
                if self.tokenizer is None:
                    raise ValueError("align: text as a string needs a checkpoint with a tokenizer; pass token ids")
                t = self.tokenizer.encode(" " + t.strip(), add_special_tokens=False).ids
            ids.append([int(v) for v in t])
        times = self.model.align_ids(audios, sample_rate, ids)
        return [self._words(t, tt, 0, 0.0) for t, tt in zip(ids, times)]

    def _run(self, audios, sample_rate: int, scored: bool = False, detailed: bool = False, single: bool = False) -> List[SttDetail]:
        """The one place where the configuration picks the native call; the public methods are projections of what it returns.
        ``timestamps``: the seek call, whatever is asked.  ``_ex``, or every field asked for (``detailed``): ``transcribe_ids_ex``.
        Else a width above 1, or a score asked for (``scored``): the beam call (width 1: the greedy ids, scored).  Else greedy:
        the single-clip call for ``single`` (``audios`` is that clip alone), the batched call otherwise."""
        from .validation import window_is_silent
        if self.timestamps:
            out = []
            clips = self._seek(audios, sample_rate)
            for c, lines in zip(clips, self._fallback_lines(clips)):
                dropped = sum(1 for w in c.windows if window_is_silent(w.no_speech_prob, w.avg_logprob, self.no_speech_threshold, self.logprob_threshold))
                ns = [w.no_speech_prob for w in c.windows if w.no_speech_prob == w.no_speech_prob]
                out.append(SttDetail(self._joined(c), c.ids, c.score, self.cfg.language_code(c.language) or str(c.language), c.language_prob,
                                     max(ns) if ns else float("nan"), dropped, **self._fallback_fields(lines),
                                     prompt_len=[w.prompt_len for w in c.windows] if self.prompted else []))
            return out
        if not (self._ex or detailed):
            if self.beam_size > 1 or scored:
                ids, scores = self.model.transcribe_ids_beam(audios, sample_rate, self.beam_size)
                return [SttDetail(self._text(i), i, s) for i, s in zip(ids, scores)]
            ids = [self.model.transcribe_ids(audios[0], sample_rate)] if single else self.model.transcribe_ids_batch(audios, sample_rate)
            return [SttDetail(self._text(i), i) for i in ids]
        # (under a fallback policy a model without languages comes here too: it has no probe pass, and reports no no-speech probability)
        kw = {"no_speech": False} if self.fallback and not self.cfg.languages else {}
        clips = self.model.transcribe_ids_ex(audios, sample_rate, self.beam_size, "auto" if self.auto else None, **kw)
        out = []
        for c, lines in zip(clips, self._fallback_lines(clips)):
            ids, at, kept, dropped = [], 0, [], 0
            for w in c.windows:
                own = c.ids[at:at + w.n_ids]                          # (a max_tokens cut leaves the last windows short)
                at += w.n_ids
                if window_is_silent(w.no_speech_prob, w.avg_logprob, self.no_speech_threshold, self.logprob_threshold):
                    dropped += 1
                else:
                    ids += own
                    kept.append(w)
            over = kept or c.windows
            avg = sum(w.logprob for w in over) / sum(w.n_ids + 1 for w in over)
            out.append(SttDetail(self._text(ids), ids, avg, self.cfg.language_code(c.language) or str(c.language),
                                 c.language_prob, max(w.no_speech_prob for w in c.windows), dropped, **self._fallback_fields(lines)))
        return out

    def _text(self, ids: List[int]) -> Optional[str]:
        if self.tokenizer is not None:
            return self.tokenizer.decode(ids, skip_special_tokens=True).strip()
        return " ".join(f"<{i}>" for i in ids)

    def ids(self, audio, sample_rate: int) -> List[int]:
        return self._run([audio], sample_rate, single=True)[0].ids

    def ids_batch(self, audios, sample_rate: int) -> List[List[int]]:
        return [d.ids for d in self._run(audios, sample_rate)]

    def batch_scored(self, audios, sample_rate: int) -> List[Tuple[Optional[str], float]]:
        """The texts of a chunk of segments with their confidence: the average log-probability per emitted token of the chosen
        hypothesis (0 is certain).  One native call, beam search of the configured width (width 1: the greedy ids, scored)."""
        return [(d.text, d.avg_logprob) for d in self._run(audios, sample_rate, scored=True)]

    def batch_detailed(self, audios, sample_rate: int) -> List[SttDetail]:
        """A chunk of segments from one native call (``transcribe_ids_ex``) with everything it reports: per clip the text and ids
        with silent windows left out, the language the prefix carried and its probability, the largest no-speech probability of its
        windows and how many windows the silence rule dropped."""
        return self._run(audios, sample_rate, detailed=True)

    def __call__(self, audio, sample_rate: int) -> Optional[str]:
        return self._run([audio], sample_rate, single=True)[0].text

    def batch(self, audios, sample_rate: int) -> List[Optional[str]]:
        """The texts of a chunk of segments from one native call (the provider's ``_chunk_texts``): per clip what ``__call__``
        returns for it (in timestamp mode: its segments' texts joined)."""
        return [d.text for d in self._run(audios, sample_rate)]

    def close(self) -> None:
        self.model.close()
