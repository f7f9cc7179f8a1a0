"""The voice bank's host side: the row plan of a multi-voice generation (voice_plan.h through rt_debug_voice_row_plan, which touches
no GPU), the configuration struct that carries max_voices in a field that was reserved, and the ABI version."""
import ctypes as C

import pytest

from rho_tts_amd import _native
from rho_tts_amd._native_model import RtModelConfig, rt_config
from rho_tts_amd import config


@pytest.fixture(scope="module")
def lib():
    return _native.load_library()


class Plan:
    """A run as generate.hip keeps it: the state arrays of rt_debug_voice_row_plan."""

    def __init__(self, lib, voices, max_rows):
        self.lib, self.voices, self.n = lib, list(voices), len(voices)
        self.v = (C.c_int32 * self.n)(*self.voices)
        self.row_item = (C.c_int32 * max_rows)()
        self.block_voice = (C.c_int32 * ((max_rows + 3) // 4))()
        self.placed = (C.c_int32 * self.n)()
        self.rows = lib.rt_debug_voice_row_plan(self.v, self.n, max_rows, 1, self.row_item, self.block_voice, self.placed, None)
        self.check()

    def items(self):
        return list(self.row_item[: self.rows])

    def blocks(self):
        return list(self.block_voice[: (self.rows + 3) // 4])

    def waiting(self):
        return [i for i in range(self.n) if not self.placed[i]]

    def finish(self, *items):
        for r in range(self.rows):
            if self.row_item[r] in items:
                self.row_item[r] = -1

    def hand_over(self):
        rev = C.c_int32()
        n = self.lib.rt_debug_voice_row_plan(self.v, self.n, self.rows, 0, self.row_item, self.block_voice, self.placed, C.byref(rev))
        self.check()
        return n, rev.value

    def check(self):
        """Every 4-row block holds one voice - the block's; no item twice."""
        on_rows = [it for it in self.items() if it >= 0]
        assert len(on_rows) == len(set(on_rows))
        for r, it in enumerate(self.items()):
            if it >= 0:
                assert self.voices[it] == self.block_voice[r // 4], (r, it, self.items(), self.blocks())
                assert self.placed[it]


@pytest.mark.parametrize("n,max_rows", [(1, 8), (3, 8), (8, 8), (13, 8), (5, 128), (128, 128), (200, 64), (7, 6)])
def test_one_voice_plans_the_layout_a_run_always_had(lib, n, max_rows):
    for voice in (0, 3):
        p = Plan(lib, [voice] * n, max_rows)
        assert p.rows == min(n, max_rows)
        assert p.items() == list(range(p.rows))
        assert p.waiting() == list(range(p.rows, n))
    # a hand-over: the next items in array order on the free rows in row order
    if n >= max_rows + 2:
        p.finish(2, 5)
        want = list(range(max_rows))
        want[2], want[5] = max_rows, max_rows + 1
        assert p.hand_over() == (2, 0) and p.items() == want


def test_an_item_waits_until_a_block_is_entirely_free(lib):
    p = Plan(lib, [0, 0, 0, 0, 0, 1], 8)
    assert p.rows == 8 and p.items() == [0, 1, 2, 3, 4, -1, -1, -1] and p.blocks() == [0, 0] and p.waiting() == [5]
    p.finish(0, 1, 2)                                  # free rows, but in blocks of voice 0 that still hold an item
    assert p.hand_over() == (0, 0) and p.waiting() == [5]
    p.finish(4)                                        # block 1 is entirely free: it is re-voiced
    assert p.hand_over() == (1, 1)
    assert p.items() == [-1, -1, -1, 3, 5, -1, -1, -1] and p.blocks() == [0, 1] and p.waiting() == []


def test_three_voices_use_three_blocks(lib):
    p = Plan(lib, [0, 1, 2], 12)
    assert p.items() == [0, -1, -1, -1, 1, -1, -1, -1, 2] and p.rows == 9 and p.blocks() == [0, 1, 2]
    assert p.rows <= 12 and p.waiting() == []


def test_order_is_kept_within_a_voice_and_another_voice_may_pass(lib):
    voices = [0, 0, 0, 0, 0, 0, 1, 0, 1]
    p = Plan(lib, voices, 8)
    # items 0..3 fill block 0, 4 and 5 open block 1 for voice 0; 6 (voice 1) finds no block; 7 joins block 1; 8 waits behind 6
    assert p.items() == [0, 1, 2, 3, 4, 5, 7, -1] and p.waiting() == [6, 8]
    p.finish(4, 5, 7)
    assert p.hand_over() == (2, 1)
    assert p.items() == [0, 1, 2, 3, 6, 8, -1, -1] and p.blocks() == [0, 1]
    # voice 0 again, behind voice 1 in block 1: it may not join, and takes block 0 once that is free - in array order
    q = Plan(lib, [1, 1, 1, 1, 0, 0, 0, 0, 0, 1, 0], 8)
    assert q.items() == [0, 1, 2, 3, 4, 5, 6, 7] and q.waiting() == [8, 9, 10]
    q.finish(5)
    assert q.hand_over() == (1, 0) and q.items()[5] == 8 and q.waiting() == [9, 10]
    q.finish(0)
    assert q.hand_over() == (1, 0) and q.items()[0] == 9 and q.waiting() == [10]
    q.finish(4, 6)
    assert q.hand_over() == (1, 0) and q.items()[4] == 10


def test_rows_never_exceed_max_rows_and_blocks_stay_pure(lib):
    import random
    rng = random.Random(5)
    for trial in range(40):
        n, max_rows = rng.randint(1, 40), rng.choice([1, 3, 4, 6, 8, 12, 16, 33])
        voices = [rng.randint(0, 3) for _ in range(n)]
        p = Plan(lib, voices, max_rows)
        assert 1 <= p.rows <= max_rows
        if p.waiting():
            assert p.rows == max_rows
        seen = []
        for _ in range(4 * n + 4):                     # finish a random busy row, hand over, until everything has had a row
            busy = [it for it in p.items() if it >= 0]
            seen += [it for it in busy if it not in seen]
            if not busy:
                break
            p.finish(rng.choice(busy))
            p.hand_over()
        assert sorted(seen) == list(range(n)), (voices, max_rows)
        for v in set(voices):                          # array order within a voice = order of first appearance on a row
            assert [it for it in seen if voices[it] == v] == [it for it in range(n) if voices[it] == v]


def test_bad_arguments_are_refused(lib):
    v = (C.c_int32 * 2)(0, 8)
    a, b, c = (C.c_int32 * 8)(), (C.c_int32 * 2)(), (C.c_int32 * 2)()
    assert lib.rt_debug_voice_row_plan(v, 2, 8, 1, a, b, c, None) == -1            # voice 8
    v[1] = 1
    assert lib.rt_debug_voice_row_plan(v, 2, 0, 1, a, b, c, None) == -1 and lib.rt_debug_voice_row_plan(v, 2, 129, 1, a, b, c, None) == -1
    assert lib.rt_debug_voice_row_plan(v, 0, 8, 1, a, b, c, None) == -1 and lib.rt_debug_voice_row_plan(None, 2, 8, 1, a, b, c, None) == -1


def test_the_struct_keeps_its_size_and_the_abi_its_version(lib):
    """max_voices travels in rt_model_config.reserved[0]: the struct is the 320 bytes it was before the bank."""
    assert C.sizeof(RtModelConfig) == 320
    assert lib.rt_abi_version() == 6
    cfg = config.tiny()
    one, four = rt_config(cfg, 4, 256, 64), rt_config(cfg, 4, 256, 64, max_voices=4)
    assert list(one.reserved) == [0, 0, 0, 0] and list(four.reserved) == [4, 0, 0, 0]
    assert bytes(one) == bytes(rt_config(cfg, 4, 256, 64, max_voices=1))
    for name in ("rt_voice_capacity", "rt_voice_select", "rt_voice_clear", "rt_generate_item_voices", "rt_generate_revoiced_blocks",
                 "rt_debug_attention_fused_voices", "rt_debug_voice_row_plan"):
        assert hasattr(lib, name), name


# ------------------------------------------------------------------------------------------------ the provider's voices= rules
# (a fake engine, in the pattern of tests/test_pipeline_host.py: no GPU)
import numpy as np
import torch

from rho_tts_amd import api
from rho_tts_amd.provider import BatchedPipeline, MI355XQwenTTS


class FakeEngine:
    """What MI355XQwenTTS asks of an engine: a named bank and synthesize(..., voices=)."""

    def __init__(self, max_voices):
        import types
        self.max_voices, self.voices, self.voice, self.calls = max_voices, {}, "own", []
        self.cfg = types.SimpleNamespace(sample_rate=24000, hf_max_position_embeddings=0)

    def conditioning_from_audio(self, audio, text, language):
        return ("cond", audio, text, language)

    def free_voice_entry(self):
        taken = {i for i, _ in self.voices.values()}
        return next(i for i in range(1, self.max_voices) if i not in taken)

    def add_voice(self, name, cond):
        self.voices[name] = (self.free_voice_entry(), cond)

    def remove_voice(self, name):
        del self.voices[name]

    def synthesize(self, texts, seed=0, item_ids=None, cancel_flag=None, stats=None, voices=None):
        self.calls.append((list(texts), list(item_ids) if item_ids is not None else None, None if voices is None else list(voices)))
        return [torch.full((2400,), 0.1 * (1 + len(t) % 5)) for t in texts]


def provider(max_voices=3, **kw):
    t = MI355XQwenTTS(reference_audio="own.wav", reference_text="own words", max_voices=max_voices, max_iterations=1, **kw)
    t._engine = FakeEngine(max_voices)
    t._ensure_voice = lambda eng: None
    return t


def test_voices_are_checked_before_anything_is_launched():
    t = provider()
    t.add_voice("b", "b.wav", "b words")
    eng = t._engine
    for bad in (["b"], ["b", None, "b", None], ["nobody", None, None], "nobody"):
        with pytest.raises(ValueError):
            t.generate(["one.", "two.", "three."], voices=bad)
        with pytest.raises(ValueError):
            t._generate_audio(["one.", "two.", "three."], voices=bad)
    assert eng.calls == [] and eng.voices == {}
    with pytest.raises(ValueError):
        next(iter(t.stream("one.", voice="nobody")))
    # the mode rules of the constructor, and the bank's size
    with pytest.raises(ValueError):
        t.add_voice("c", speaker="ryan")                       # a Base model clones: it needs reference audio
    with pytest.raises(ValueError):
        t.add_voice("c", "c.wav")                              # ... and its transcript
    t.add_voice("c", "c.wav", "c words")
    with pytest.raises(ValueError):
        t.add_voice("d", "d.wav", "d words")                   # max_voices = 3: the constructor's voice and two named ones
    t.add_voice("c", "c2.wav", "c words")                      # replacing a name is not adding one
    assert t.voices == ["b", "c"]
    t.remove_voice("c")
    with pytest.raises(ValueError):
        t.remove_voice("c")
    with pytest.raises(ValueError):
        MI355XQwenTTS(reference_audio="a.wav", reference_text="a", max_voices=9)
    custom = MI355XQwenTTS(speaker="vivian", model_path="x/CustomVoice", max_voices=2)
    with pytest.raises(ValueError):
        custom.add_voice("r", reference_audio="r.wav", reference_text="r")      # a CustomVoice model needs a named speaker
    custom.add_voice("r", speaker="ryan")


def test_none_entries_mean_the_constructors_voice_and_a_name_serves_every_text():
    t = provider()
    t.add_voice("b", "b.wav", "b words")
    eng = t._engine
    out = t._generate_audio(["one.", "two.", "three."], item_ids=[5, 6, 7], voices=[None, "b", None])
    assert len(out) == 3 and eng.calls[-1] == (["one.", "two.", "three."], [5, 6, 7], [None, "b", None])
    assert list(eng.voices) == ["b"] and eng.voices["b"][1] == ("cond", "b.wav", "b words", "English")
    t._generate_audio(["one.", "two."], voices="b")
    assert eng.calls[-1][2] == ["b", "b"]
    t._generate_audio(["one.", "two."], voices=[None, None])   # names nobody: the call every caller made before the bank
    assert eng.calls[-1][2] is None
    t._generate_audio("one.")
    assert eng.calls[-1][2] is None


class Pipe(BatchedPipeline, api.BaseTTS):
    """The batched pipeline over a recording _generate_audio, with scripted validators."""

    def __init__(self, **kw):
        super().__init__(device="cpu", **kw)
        self.batch_size, self.max_iterations, self.seen, self.scored = 16, 3, [], []

    def _finish_items(self, items):
        return [(torch.cat(list(it)), 1.0, True) for it in items]

    def _generate_audio(self, text, **kwargs):
        texts = [text] if isinstance(text, str) else list(text)
        self.seen.append((texts, kwargs.get("voices", "absent")))
        out = [torch.full((1200,), float(len(t))) for t in texts]
        return out[0] if isinstance(text, str) else out

    @property
    def sample_rate(self):
        return 24000


def test_segments_inherit_their_texts_voice_and_foreign_voices_are_not_scored_for_drift():
    t = Pipe()
    t.max_chars_per_segment, t.force_sentence_split = 12, True
    texts = ["Aa aa aa. Bb bb bb. Cc cc.", "Dd dd dd.", "Ee ee ee. Ff ff ff."]
    plans = t._plan_texts(texts, api.CancellationToken())
    assert len(plans[0]) >= 2 and len(plans[2]) >= 2

    def scorer(audio, sr):
        t.scored.append(float(audio[0]))
        return 0.05
    t.drift_scorer = scorer
    t.transcriber = None
    t._call_voices = ["b", None, "b"]
    try:
        res = t._run_plans(plans, [0, 1, 2], api.CancellationToken())
    finally:
        t._call_voices = None
    segs, voices = t.seen[0]
    want = [v for i, v in enumerate(["b", None, "b"]) for _ in plans[i]]
    assert segs == [s for p in plans for s in p] and voices == want
    # drift: only the constructor's voice is scored, and only its item carries drift_prob
    assert t.scored == [float(len(s)) for s in plans[1]]
    assert "drift_prob" not in res[0][2] and "drift_prob" not in res[2][2] and res[1][2]["drift_prob"] == 0.05
    assert all("decay_ratio" in r[2] for r in res)
    # a call without voices hands _generate_audio no voices keyword at all
    t.seen.clear()
    t._run_plans(plans, [0, 1, 2], api.CancellationToken())
    assert t.seen[0][1] == "absent"


def test_generate_with_voices_runs_the_inherited_body_and_logs_the_drift_notice_once(caplog):
    """The public path: generate(texts, voices=...) -> the inherited BaseTTS.generate -> pipeline -> _generate_audio(voices=...), the
    call's voices held as instance state meanwhile and gone afterwards; the notice about drift comes once per call, retries or not."""
    import logging
    t = provider(max_voices=2)
    t.max_iterations, t.max_decay_retries = 2, 3
    t.add_voice("b", "b.wav", "b words")
    attempts = []

    def finish(items):                                         # the first two attempts decay: the texts are regenerated whole
        attempts.append(len(items))
        return [(torch.cat(list(it)), 1.0, len(attempts) >= 3) for it in items]
    t._finish_items = finish
    t.drift_scorer = lambda audio, sr: 0.05
    texts = ["The first text.", "The second text.", "The third text."]
    with caplog.at_level(logging.INFO):
        res = t.generate(texts, voices=[None, "b", None])
    assert len(res) == 3 and all(r is not None for r in res) and len(attempts) == 3
    assert t._call_voices is None
    calls = t._engine.calls
    assert len(calls) == 3 and all(c[0] == texts and c[2] == [None, "b", None] for c in calls)
    assert sum("accent drift is scored for the provider's own voice only" in r.getMessage() for r in caplog.records) == 1
    # ... and a call without voices afterwards is a plain one
    t.generate(texts[:1])
    assert t._engine.calls[-1][2] is None
