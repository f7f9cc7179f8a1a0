"""A serving session through the provider (MI355XQwenTTS.serve): requests from two threads with two voices join one decode batch; every
result is what generate() gives the text alone, every streamed piece what stream() gives it alone on a fresh instance - for the
bank-voice stream, which stream() refuses with chunk sizes, what Engine.stream_wav + rt_stream_chunk give."""
import threading

import pytest
import torch

pytestmark = pytest.mark.gpu

WAIT = 60.0
FIRST, NEXT = 6, 10
MULTI = "First sentence of eight words is right here. Second one is a little bit shorter."
PLAIN = "A plain request in the second voice. It has two segments too."
LONG = "This one is cancelled half way through its many many words and never reaches the end of what it has to say."


def provider(**kw):
    from rho_tts_amd.provider import MI355XQwenTTS
    t = MI355XQwenTTS(device="cuda", speaker="Vivian", model_path="x/CustomVoice-small", batch_size=8, max_iterations=1, max_voices=2, **kw)
    t.force_sentence_split = True
    t.max_decay_retries = 1                                   # (a session does not retry: compare with one pass)
    t.add_voice("r", speaker="Ryan", language="chinese")
    return t


def bank_stream_alone(f, text, voice):
    """the pieces of sub-segment streaming with a bank voice, from the engine's own streaming calls, one segment after the other"""
    eng = f._load_engine()
    with f._lock:
        f._ensure_voice(eng)
        f._ensure_bank(eng, [voice])
    params, out = f._post_params(0), []
    for seg in f._split_text_into_segments(f._apply_phonetic_mapping(text), f._compute_max_chars()):
        state, started = [0.0, 1.0], False
        for raw, last in eng.stream_wav(seg, seed=int(f.seed), item_id=0, first_chunk=FIRST, chunk=NEXT, voice=voice):
            if not raw.numel():
                continue
            audio = eng.ctx.stream_chunk(params, raw, state, first=not started, last=last)
            if not started:
                if state[1] <= 0.0:
                    continue
                started = True
            if audio.numel():
                out.append(audio)
    return out


def test_requests_from_two_threads_get_what_they_get_alone():
    t, f = provider(), provider()
    try:
        want_plain = t.generate(PLAIN, voices="r")
        want_own = t.generate(MULTI)
        assert want_plain.segments_count == 2 and want_own.segments_count == 2
        f.stream_chunk_frames, f.stream_next_chunk_frames = FIRST, NEXT
        want_pieces = list(f.stream(MULTI))
        with pytest.raises(ValueError):
            list(f.stream(MULTI, voice="r"))                     # plain stream() keeps its restriction ...
        want_bank = bank_stream_alone(f, MULTI, "r")             # ... a session lifts it
        assert len(want_pieces) > 4 and len(want_bank) > 4
        handles, errors = {}, []

        def listener(name, text, **kw):
            try:
                handles[name] = s.submit(text, **kw)
            except Exception as e:  # noqa: BLE001
                errors.append(e)
        with t.serve(voices=["r"], stream_chunk_frames=FIRST, stream_next_chunk_frames=NEXT, timeout=WAIT) as s:
            threads = [threading.Thread(target=listener, args=("stream", MULTI), kwargs=dict(stream=True)),
                       threading.Thread(target=lambda: (listener("plain", PLAIN, voice="r"), listener("cancel", LONG, voice="r", stream=True)))]
            for th in threads:
                th.start()
            for th in threads:
                th.join(WAIT)
            assert not errors and sorted(handles) == ["cancel", "plain", "stream"]
            it = iter(handles["cancel"])
            first = next(it)
            handles["cancel"].cancel()
            assert first.audio.numel() > 0 and len(list(it)) < 6
            own = s.submit(MULTI)                                  # joins while the others decode
            bank = s.submit(MULTI, voice="r", stream=True)
            got_pieces = list(handles["stream"])
            got_plain = handles["plain"].result(timeout=WAIT)
            got_bank = list(bank)
            got_own = own.result(timeout=WAIT)
            with pytest.raises(RuntimeError, match="session"):
                t.generate(PLAIN)
            with pytest.raises(RuntimeError, match="session"):
                list(t.stream(PLAIN))
            with pytest.raises(RuntimeError, match="session"):
                t.add_voice("x", speaker="Ryan")
            from rho_tts_amd.serving import RequestCancelled
            with pytest.raises(RequestCancelled):
                handles["cancel"].result(timeout=WAIT)
        assert len(got_pieces) == len(want_pieces) and all(torch.equal(a.audio, b.audio) for a, b in zip(got_pieces, want_pieces))
        assert len(got_bank) == len(want_bank) and all(torch.equal(a.audio, b) for a, b in zip(got_bank, want_bank))
        for got, want in ((got_plain, want_plain), (got_own, want_own)):
            assert torch.equal(got.audio, want.audio) and got.segments_count == want.segments_count and got.decay_ratio == want.decay_ratio
            assert got.sample_rate == want.sample_rate and got.duration_sec == want.duration_sec
        assert not torch.equal(got_own.audio[: 1000], got_plain.audio[: 1000])
        again = t.generate(PLAIN, voices="r")                      # the session is closed: generate() is back, and gives what it gave
        assert torch.equal(again.audio, want_plain.audio)
    finally:
        t.close()
        f.close()


def test_a_spent_horizon_is_reopened_by_the_worker():
    """a horizon that holds three or four segments: the library refuses the next submit with RT_ERR_LENGTH, the worker drains, reopens
    and goes on - no request is lost, and each is what generate() gives it alone"""
    t = provider()
    try:
        want = t.generate(PLAIN, voices="r")
        eng = t._load_engine()
        segs = t._split_text_into_segments(t._apply_phonetic_mapping(PLAIN), t._compute_max_chars())
        fmax = max(eng.frames_actual(x, len(eng.tokenizer.encode(x))) for x in segs)
        with t.serve(rows=4, voices=["r"], horizon=4 * fmax + 40, timeout=WAIT) as s:
            hs = [s.submit(PLAIN, voice="r") for _ in range(5)]
            got = [h.result(timeout=WAIT) for h in hs]
            assert s.reopened >= 1
            assert eng.model.cadence() == s.run.every == 4
        assert all(torch.equal(g.audio, want.audio) for g in got)
    finally:
        t.close()
