"""Text-match scoring of a transcription against the text that was to be spoken - the host-side half of the reference's
STT validation (validation/stt/stt_validator.py: ``_normalize_text`` :22-39, ``_levenshtein_distance`` :151-169,
``_fuzzy_word_match`` :172-185, ``calculate_text_similarity`` :188-232, ``validate_audio_text_match`` :235-260), restated so
that a provider can validate a waveform it still holds in HBM without the temp-WAV round trip of base_tts.py:821-830: the
transcriber is a callable on the tensor (``MI355XQwenTTS.transcriber``), the scoring below is pure string work.

Pinned by tests/golden/textsim_golden.json (pairs scored by the reference's own function).  Number normalisation
(number_normalizer.py, NeMo inverse text normalisation) is NOT restated: its dependency is absent offline, the reference
itself degrades to "warn and continue" when it fails (:27-31), and the fixtures therefore contain no numerals.
"""
from __future__ import annotations

import re
from difflib import SequenceMatcher
from typing import Callable, Optional, Tuple


def normalize_text(text: str, number_normalizer: Optional[Callable[[str], str]] = None) -> str:
    if number_normalizer is not None:
        try:
            text = number_normalizer(text)
        except Exception:  # noqa: BLE001  (the reference warns and goes on)
            pass
    text = text.lower()
    text = re.sub(r"\b(the|a|an)\b", " ", text)
    text = text.replace("-", " ")
    text = re.sub(r"[^\w\s']", " ", text)
    text = re.sub(r"\s+", " ", text)
    return text.strip()


def levenshtein_distance(s1: str, s2: str) -> int:
    if len(s1) < len(s2):
        s1, s2 = s2, s1
    if not s2:
        return len(s1)
    prev = list(range(len(s2) + 1))
    for i, c1 in enumerate(s1):
        cur = [i + 1]
        for j, c2 in enumerate(s2):
            cur.append(min(prev[j + 1] + 1, cur[j] + 1, prev[j] + (c1 != c2)))
        prev = cur
    return prev[-1]


def fuzzy_word_match(w1: str, w2: str, max_distance: int = 2) -> bool:
    if w1 == w2:
        return True
    if len(w1) < 3 or len(w2) < 3:
        return False
    limit = max_distance + 1 if (len(w1) > 8 or len(w2) > 8) else max_distance
    return levenshtein_distance(w1, w2) <= limit


def calculate_text_similarity(original_text: str, transcribed_text: str, number_normalizer=None) -> float:
    """max(Jaccard, matched / original words, character sequence ratio) over normalised texts, fuzzy word matches counted."""
    o, t = normalize_text(original_text, number_normalizer), normalize_text(transcribed_text, number_normalizer)
    ow, tw = set(o.split()), set(t.split())
    if not ow or not tw:
        return 0.0
    fuzzy = 0
    # (set iteration order only decides WHICH transcribed word a fuzzy match pairs with, never the count: every original word
    #  counts at most once and transcribed words are not consumed - exactly the reference's loop)
    for a in ow - tw:
        if any(fuzzy_word_match(a, b) for b in tw - ow):
            fuzzy += 1
    total = len(ow & tw) + fuzzy
    union = len(ow | tw)
    return max(total / union if union else 0.0, total / len(ow), SequenceMatcher(None, o, t).ratio())


def validate_text_match(transcribed: Optional[str], expected_text: str, threshold: float = 0.85) -> Tuple[bool, float, Optional[str]]:
    """(is_valid, similarity, transcription); a failed transcription passes with similarity 0.0 (:249-252)."""
    if transcribed is None:
        return True, 0.0, None
    sim = calculate_text_similarity(expected_text, transcribed)
    return sim >= threshold, sim, transcribed


def window_is_silent(no_speech_prob: float, avg_logprob: float, no_speech_threshold: Optional[float] = 0.6, logprob_threshold: Optional[float] = -1.0) -> bool:
    """The silence rule of Whisper's transcribers for one 30-s window: silent - its ids are dropped - when the no-speech probability
    is ABOVE ``no_speech_threshold`` and the hypothesis' average log-probability (cumulative log-probability / (ids + 1)) is BELOW
    ``logprob_threshold``: "probably silence" and "low confidence" together (transformers generation_whisper.py: ``_need_fallback``
    sets should_skip on exactly this pair; faster-whisper's transcribe.py applies the same test; defaults 0.6 and -1.0).
    ``no_speech_threshold`` None switches the rule off; ``logprob_threshold`` None leaves the no-speech test alone, as in
    faster-whisper.  A NaN is never above or below anything: such a window is kept."""
    if no_speech_threshold is None or not no_speech_prob > no_speech_threshold:
        return False
    return logprob_threshold is None or avg_logprob < logprob_threshold


# ---------------------------------------------------------------------------------------------- temperature fallback
# The rule of Whisper's transcribers that decides whether a decoded window is decoded again at the next temperature (DESIGN.md
# section 5, "temperature fallback"; faster-whisper's generate_with_fallback, transformers' _need_fallback, openai-whisper's
# decode_with_fallback), restated: the native loop (csrc/stt.hip stt_fallback_group) applies the same statements, and the compression
# ratio reaches it as a callback, since it is zlib's.
def compression_ratio_ids(ids, vocab: int) -> float:
    """transformers' ``_retrieve_compression_ratio``: every id as ``int(log2(vocab) / 8) + 1`` little-endian bytes, the length of
    those bytes over the length of their zlib compression."""
    import math
    import zlib
    length = int(math.log2(int(vocab)) / 8) + 1
    raw = b"".join(int(t).to_bytes(length, "little") for t in ids)
    return len(raw) / len(zlib.compress(raw))


def compression_ratio_text(text: str) -> float:
    """faster-whisper's ``get_compression_ratio`` on a window's text: the UTF-8 bytes of the stripped text over their zlib compression."""
    import zlib
    raw = text.strip().encode("utf-8")
    return len(raw) / len(zlib.compress(raw))


def needs_fallback(compression_ratio: Optional[float], avg_logprob: float, no_speech_prob: float = float("nan"),
                   compression_ratio_threshold: Optional[float] = 2.4, logprob_threshold: Optional[float] = -1.0,
                   no_speech_threshold: Optional[float] = None) -> bool:
    """Whether one attempt at a window must be followed by another: its text compresses too well (``compression_ratio`` ABOVE its
    threshold) or its average log-probability is BELOW its threshold - unless the window is silence (``window_is_silent`` with both
    thresholds set), which the caller's silence rule deals with.  A threshold of None, or no ratio, switches that test off."""
    needs = False
    if compression_ratio_threshold is not None and compression_ratio is not None and compression_ratio > compression_ratio_threshold:
        needs = True
    if logprob_threshold is not None and avg_logprob < logprob_threshold:
        needs = True
    if no_speech_threshold is not None and logprob_threshold is not None and no_speech_prob > no_speech_threshold and avg_logprob < logprob_threshold:
        needs = False
    return needs


def prompt_for_window(history, reset_mark: int, cap: int):
    """The prompt a window decodes behind ("conditioning on previous text"; faster-whisper's ``get_prompt`` on
    ``all_tokens[prompt_reset_since:]``): the clip's history behind the reset mark, cut to its last ``cap`` ids
    (``cap = n_text_ctx // 2 - 1``).  Empty: the window decodes behind the timestamp-mode prefix alone."""
    tail = [int(t) for t in history[int(reset_mark):]]
    return tail[len(tail) - min(len(tail), int(cap)):]


def history_after_window(history, reset_mark: int, segments, silent: bool = False, condition_on_previous: bool = True, temperature: float = 0.0,
                         reset_on_temperature: Optional[float] = 0.5):
    """(history, reset mark) of a clip after one window.  ``segments``: the window's closed segments in order as (start tick, end
    tick, text ids, every id of the slice with its timestamps) - a discarded tail is no segment.  A silent window changes nothing.
    Otherwise every segment with a duration and at least one text id adds all of its ids, and the mark moves to the end of the
    history when conditioning is off or the window's chosen attempt ran at a ``temperature`` above ``reset_on_temperature`` (None:
    never).  The native loop (csrc/stt.hip stt_transcribe_seek) applies the same statements."""
    history = [int(t) for t in history]
    if silent:
        return history, int(reset_mark)
    for start, end, text, raw in segments:
        if start != end and len(text):
            history += [int(t) for t in raw]
    if not condition_on_previous or (reset_on_temperature is not None and temperature > reset_on_temperature):
        reset_mark = len(history)
    return history, int(reset_mark)


def pick_attempt(attempts, compression_ratio_threshold: Optional[float] = 2.4) -> int:
    """The attempt that stands when every temperature failed: ``attempts`` is a list of (compression_ratio or None, avg_logprob) in the
    order they were made; the largest average among those within the compression threshold wins, among all when none is within it,
    and the earliest on a tie."""
    def within(r):
        return compression_ratio_threshold is None or r is None or not r > compression_ratio_threshold
    pool = [k for k, (r, _) in enumerate(attempts) if within(r)] or list(range(len(attempts)))
    best = pool[0]
    for k in pool[1:]:
        if attempts[k][1] > attempts[best][1]:
            best = k
    return best
