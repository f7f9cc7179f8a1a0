"""Host side of the word times ("word times"), no GPU: the reference of tests/stt_align_ref.py on a planted matrix,
the word grouping restated from OpenAI's tokenizer on hand-made id / decode tables, the configuration fields, the argument rules."""
import dataclasses

import numpy as np
import pytest
import torch

from rho_tts_amd import stt as S
from tests import stt_align_ref as R


@pytest.mark.parametrize("n,F", [(1, 1), (1, 9), (5, 5), (13, 65), (40, 300)])
def test_reference_finds_a_planted_staircase(n, F):
    M, first = R.planted_matrix(n, F, seed=n * 1000 + F)
    assert np.array_equal(R.dtw_frames(M), first)


def test_reference_matrix_on_a_constant_column_and_a_short_window():
    W = torch.tensor([[[1.0, 5.0, 2.0], [3.0, 5.0, 0.0]]])                  # one head, two rows, three frames: width 7 leaves it unfiltered
    M = R.matrix(W, 7)
    assert torch.equal(M, torch.tensor([[-1.0, 0.0, 1.0], [1.0, 0.0, -1.0]]))
    W4 = torch.tensor([[[0.0, 1.0, 9.0, 3.0], [2.0, 0.0, 1.0, 0.0]]])      # four frames: filtered, the reflect pad reaches index 3
    z = torch.tensor([-1.0, 1.0, 1.0, 1.0])                                 # row 0's z; padded: z3 z2 z1 | z0 z1 z2 z3 | z2 z1 z0
    want = [sorted([z[3], z[2], z[1], z[0], z[1], z[2], z[3]])[3], sorted([z[2], z[1], z[0], z[1], z[2], z[3], z[2]])[3]]
    assert [float(v) for v in R.matrix(W4, 7)[0, :2]] == [float(v) for v in want]


# a hand-made vocabulary: id -> bytes; decode joins the bytes and reads them as UTF-8 the way tokenizers do (errors="replace")
PIECES = {0: b" Hello", 1: b" wor", 2: b"ld", 3: b",", 4: b" (", 5: b"yes", 6: b")", 7: b"!", 8: b" caf", 9: b"\xc3", 10: b"\xa9", 11: b" \"", 12: b"ok", 13: b"\"", 14: b" yes"}


def decode(ids):
    return b"".join(PIECES[int(i)] for i in ids).decode("utf-8", errors="replace")


def test_leading_space_opens_a_word_and_punctuation_merges_to_both_sides():
    ids = [0, 1, 2, 3, 4, 5, 6, 7, 11, 12, 13]
    spaces = S.split_tokens_on_spaces(ids, decode)
    assert [t for t, _ in spaces] == [" Hello", " world", ",", " (yes", ")", "!", " \"ok", "\""]
    assert [p for _, p in spaces][1] == [1, 2]
    words = S.group_words(ids, decode)
    assert [t for t, _ in words] == [" Hello", " world,", " (yes)!", " \"ok\""]
    assert [p for _, p in words] == [[0], [1, 2, 3], [4, 5, 6, 7], [8, 9, 10]]
    assert sorted(k for _, p in words for k in p) == list(range(len(ids)))
    # an opening bracket that stands alone (the next piece has a space of its own) joins the word behind it
    assert S.group_words([0, 4, 14, 7], decode) == [(" Hello", [0]), (" ( yes!", [1, 2, 3])]


def test_an_incomplete_utf8_piece_is_carried_over():
    ids = [8, 9, 10, 7]
    assert S.split_tokens_on_unicode(ids, decode) == [(" caf", [0]), ("é", [1, 2]), ("!", [3])]
    assert S.group_words(ids, decode) == [(" café!", [0, 1, 2, 3])]
    assert S.group_words(ids, decode, spaces=False) == [(" caf", [0]), ("é!", [1, 2, 3])]


def test_without_a_tokenizer_every_id_is_a_word():
    assert S.group_words([7, 300, 7]) == [("<7>", [0]), ("<300>", [1]), ("<7>", [2])]
    times = S.SttTokenTimes([0.0, 0.1, 0.1], [0.1, 0.1, 0.5], [0.0, -1.0, -2.0], 40)
    words = S.words_from_times([7, 300, 7], times, 0, S.group_words([7, 300, 7]), shift=2.0)
    assert [(w.word, w.start, w.end, w.ids) for w in words] == [("<7>", 2.0, 2.1, [7]), ("<300>", 2.1, 2.1, [300]), ("<7>", 2.1, 2.5, [7])]
    assert [w.probability for w in words] == pytest.approx([1.0, np.exp(-1.0), np.exp(-2.0)])
    both = S.words_from_times([1, 2], times, 1, [("x", [0, 1])])
    assert (both[0].start, both[0].end) == (0.1, 0.5) and both[0].probability == pytest.approx(np.exp(-1.5))


def test_alignment_heads_of_a_configuration():
    js = {"d_model": 384, "decoder_layers": 4, "encoder_attention_heads": 6}
    c = S.SttConfig.from_hf(js, {"alignment_heads": [[2, 2], [3, 0], [3, 2]], "median_filter_width": 5})
    assert c.alignment_heads == ((2, 2), (3, 0), (3, 2)) and c.aligned_heads == ((2, 2), (3, 0), (3, 2)) and c.median_filter_width == 5
    d = S.SttConfig.from_hf(js, {})
    assert d.alignment_heads is None and d.median_filter_width == 7
    assert d.aligned_heads == tuple((l, h) for l in (2, 3) for h in range(6))          # OpenAI's default: the upper half of the decoder
    assert S.tiny_test_config().aligned_heads == ((1, 0), (1, 1))
    assert S.SttSegment(0.0, 1.0, [1]).words is None and list(S.SttSegment.__dataclass_fields__)[-1] == "words"


def test_a_model_whose_heads_cannot_be_set_still_loads():
    """Whisper small, medium and large without `alignment_heads` (an empty or missing generation config) have 72, 192 and 320 heads in
    the upper half of the decoder, more than the native call takes: the configuration parses as before, the loader is told not to set
    them (``alignment_error``), and only the use of word times raises."""
    for d_model, layers, heads in ((768, 12, 12), (1024, 24, 16), (1280, 32, 20)):
        c = S.SttConfig.from_hf({"d_model": d_model, "decoder_layers": layers, "encoder_layers": layers, "encoder_attention_heads": heads}, {})
        assert len(c.aligned_heads) == (layers - layers // 2) * heads > 32
        assert "the default" in S.alignment_error(c) and str(len(c.aligned_heads)) in S.alignment_error(c)
    small = S.SttConfig.from_hf({"d_model": 768, "decoder_layers": 12, "encoder_attention_heads": 12}, {"alignment_heads": [[5, 3], [8, 0], [9, 9]]})
    assert S.alignment_error(small) is None and S.alignment_error(S.SttConfig()) is None and S.alignment_error(S.tiny_test_config()) is None
    for bad in (dict(alignment_heads=((4, 0),)), dict(alignment_heads=((1, 6),)), dict(alignment_heads=((1, 0), (1, 0))), dict(alignment_heads=()),
                dict(median_filter_width=6), dict(median_filter_width=33), dict(median_filter_width=0)):
        assert S.alignment_error(dataclasses.replace(S.SttConfig(), **bad)) is not None, bad
    # the loader's own lines: no native call for such a model, and the use raises with the reason
    calls = []

    class Lib:
        @staticmethod
        def rt_stt_set_alignment(handle, flat, n, width):
            calls.append((list(flat), n, width))
            return 0
    nat = object.__new__(S.NativeSTT)
    nat.lib, nat.handle = Lib(), 1
    nat.cfg = S.SttConfig.from_hf({"d_model": 768, "decoder_layers": 12, "encoder_layers": 12, "encoder_attention_heads": 12}, {})
    nat._set_alignment()
    assert calls == [] and "72 heads" in nat.alignment_error
    with pytest.raises(ValueError, match="no alignment heads.*72 heads"):
        nat.align_ids([np.zeros(10, dtype=np.float32)], 16000, [[1]])
    nat.cfg = small
    nat._set_alignment()
    assert calls == [([5, 3, 8, 0, 9, 9], 3, 7)] and nat.alignment_error is None
    nat.handle = None                                               # (nothing to destroy)


def test_argument_rules():
    with pytest.raises(ValueError, match="word_timestamps needs timestamps=True"):
        S.WhisperTranscriber(None, synthetic=True, cfg=S.tiny_test_config(), word_timestamps=True, timestamps=False)
    t = object.__new__(S.WhisperTranscriber)
    t.cfg, t.tokenizer = S.tiny_test_config(), None
    with pytest.raises(ValueError, match=r"at most 2 s \(48000 samples\)"):
        t.align([np.zeros(48001, dtype=np.float32)], 24000, [[1, 2]])
    with pytest.raises(ValueError, match="needs a checkpoint with a tokenizer"):
        t.align([np.zeros(100, dtype=np.float32)], 24000, ["hello"])
    with pytest.raises(ValueError, match="1 texts for 2 clips"):
        t.align([np.zeros(1), np.zeros(1)], 24000, [[1]])


def test_provider_word_times_names_the_missing_transcriber():
    from rho_tts_amd import provider as P
    tts = object.__new__(P.MI355XQwenTTS)
    with pytest.raises(ValueError, match="transcriber=WhisperTranscriber"):
        tts.word_times(torch.zeros(10), "hello")
