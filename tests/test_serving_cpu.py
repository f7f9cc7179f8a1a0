"""The serving scheduler (rho_tts_amd/serving.py) on the CPU, against a fake run: per-item cuts, ordering, cancellation, error
delivery, shutdown and the reopen on a spent horizon.  The yardstick for a streaming request is the loop a caller of
``stream()`` runs for that text ALONE (Engine.stream_codes / stream_wav and the provider's chunk loop), restated here over the same
fake run: a listener's pieces must not depend on who else is connected or on the tick the request arrived in."""
import threading
import zlib

import pytest
import torch

from rho_tts_amd.serving import Handle, HorizonSpent, RequestCancelled, Session, SessionClosed, piece_is_last

UP, TRIM, LEFT = 4, 2, 2          # samples per frame, samples a decode falls short of n * UP, frames of left context
WAIT = 20.0                       # every wait of a test: a defect fails, it does not hang


class FakeRun:
    """An open run in miniature.  A text is ``name:frames[:eK][:silent]``: its frame budget, an end-of-sequence frame at index K (the
    host learns of it once that frame has run), a first dozen frames of silence.  Rows are looked at before every frame; waiting
    items take free rows in submission order.  Codes are a function of (text, voice, item id, frame) alone."""

    every = 4

    def __init__(self, rows=4, horizon=10 ** 6, gate=False, fail_at=None, pause_at=None):
        self.rows, self.horizon, self.fail_at, self.pause_at = rows, horizon, fail_at, pause_at
        self.gate = threading.Event() if gate else None      # closed: step() waits for the test to open it
        self.paused = threading.Event()                        # step number pause_at has closed the gate again and waits
        self.opens = self.closes = self.steps = self.vocodes = self.posts = 0
        self.placed, self.cancelled, self.submitted = [], [], []
        self.items, self.t = [], 0

    def open(self):
        self.opens += 1
        self.items, self.t = [], 0

    def close(self):
        self.closes += 1

    def split(self, text):
        return [t for t in text.split("|") if t]

    def submit(self, text, voice, item_id):
        parts = text.split(":")
        if parts[0] == "bad":
            raise ValueError("refused: " + text)
        frames = int(parts[1])
        eos = next((int(p[1:]) for p in parts[2:] if p.startswith("e")), None)
        owed = sum(max(0, it["need"] - it["run"]) for it in self.items if not it["fin"])
        if self.t + owed + frames + 1 > self.horizon:
            raise HorizonSpent("the horizon is spent")
        base = zlib.crc32(f"{text}/{voice}/{item_id}".encode()) % 997 + 1
        total = frames if eos is None else eos
        codes = torch.tensor([[base + f, base + 2 * f] for f in range(total)], dtype=torch.int64).reshape(total, 2)
        if "silent" in parts:
            codes[:12] = 0
        self.items.append(dict(text=text, voice=voice, id=item_id, codes=codes, total=total, need=frames if eos is None else eos + 1,
                               run=0, row=None, fin=False))
        self.submitted.append((text, voice, item_id))
        return len(self.items) - 1, frames

    def _place(self):
        busy = {it["row"] for it in self.items if it["row"] is not None and not it["fin"]}
        for k, it in enumerate(self.items):
            if it["row"] is None and not it["fin"] and len(busy) < self.rows:
                it["row"] = min(set(range(self.rows)) - busy)
                busy.add(it["row"])
                self.placed.append(it["text"])

    def step(self, n):
        if self.gate is not None:
            if self.pause_at == self.steps + 1:
                self.gate.clear()
                self.paused.set()
            if not self.gate.wait(WAIT):
                raise RuntimeError("the test never opened the gate")
        self.steps += 1
        if self.fail_at == self.steps:
            raise RuntimeError("boom")
        for _ in range(n):
            self._place()
            live = [it for it in self.items if it["row"] is not None and not it["fin"]]
            if not live:
                break
            for it in live:
                it["run"] += 1
                it["fin"] = it["run"] >= it["need"]
            self.t += 1
        return all(it["fin"] for it in self.items)

    def peek(self, item, first, n):
        it = self.items[item]
        have = min(it["run"], it["total"])
        return it["codes"][first: max(first, min(have, first + n))], it["fin"]

    def cancel(self, item):
        self.items[item]["fin"] = True
        self.cancelled.append(self.items[item]["text"])

    def context(self, start):
        return LEFT if start - LEFT > 0 else start

    def samples(self, frames):
        return frames * UP

    def vocode(self, codes):
        self.vocodes += 1
        return [c[:, 0].float().repeat_interleave(UP)[: c.shape[0] * UP - TRIM] + torch.arange(c.shape[0] * UP - TRIM) % UP * 0.125 for c in codes]

    vocode_whole = vocode

    def post(self, wavs, states, flags):
        self.posts += 1
        out = []
        for w, st, (first, last) in zip(wavs, states, flags):
            if w.numel() == 0:
                out.append(w)
                continue
            if first:
                st[0], st[1] = (0.0, 0.0) if float(w.abs().max()) < 1.0 else (0.5, 2.0)      # silence: nothing measured, gain 0
            out.append(w * (st[1] or 1.0) - st[0] + (10000.0 if first else 0.0) + (0.03125 if last else 0.0))
        return out

    def finish(self, items, requests):
        return [("whole", r.voice, [w.clone() for w in segs]) for segs, r in zip(items, requests)]

    def wrap(self, wav, req):
        return wav


def alone(text, voice=None, item_id=0, first_chunk=12, chunk=36):
    """the pieces of one segment streamed by itself: the stream_codes / stream_wav / chunk loop of a caller that owns the run"""
    run = FakeRun(rows=1)
    run.open()
    item, frames = run.submit(text, voice, item_id)
    pieces, have, emitted, state, started, sent, step = [], None, 0, [0.0, 1.0], False, 0, first_chunk
    while True:
        done = run.step(step)
        codes, _ = run.peek(item, sent, frames)
        sent += int(codes.shape[0])
        if codes.shape[0]:
            start = 0 if have is None else int(have.shape[0])
            have = codes if have is None else torch.cat([have, codes])
            ctx = run.context(start)
            w = run.vocode([have[start - ctx:]])[0]
            piece = w[max(0, emitted - (start - ctx) * UP):]
            emitted += int(piece.numel())
            out = run.post([piece], [state], [(not started, done)])[0]
            if started or state[1] > 0.0:
                started = True
                if out.numel():
                    pieces.append(out)
        if done:
            return pieces
        step = chunk


def same(got, want):
    assert len(got) == len(want), (len(got), len(want))
    for a, b in zip(got, want):
        assert torch.equal(a, b)


def collect(h):
    return list(iter(h))


def test_piece_is_last_is_what_a_lone_caller_sees():
    assert piece_is_last(True, 14, 48, 14) and piece_is_last(True, 12, 12, 12)
    assert not piece_is_last(True, 12, 12, 40)          # end-of-sequence right behind the cut: not run yet when the piece goes out
    assert not piece_is_last(False, 12, 12, 40) and not piece_is_last(True, 13, 12, 13)


def test_an_item_that_starts_mid_tick_gets_the_pieces_it_gets_alone():
    run = FakeRun(rows=1, gate=True)
    with Session(run, timeout=WAIT) as s:
        a = s.submit("a:6")                             # one row: b starts at frame 6, in the middle of a 4-frame tick
        b = s.submit("b:53", stream=True)
        c = s.submit("c:30", stream=True, voice="v")    # ... and c at frame 59
        run.gate.set()
        assert a.result()[0] == "whole"
        same(collect(b), alone("b:53"))
        same(collect(c), alone("c:30", "v"))
        assert b.result() is None
    assert run.placed == ["a:6", "b:53", "c:30"]
    # the absolute cut: the pieces of a segment played back to back are as long as one decode of all its frames
    assert [int(p.numel()) for p in alone("b:53")] == [12 * UP - TRIM, 36 * UP, 5 * UP]


def test_pieces_do_not_depend_on_who_else_is_connected():
    texts = ["a:40", "b:12", "c:14", "d:49:e12", "e:30:silent", "f:5", "g:48"]
    want = [alone(t, "v" if i % 2 else None) for i, t in enumerate(texts)]
    for rows in (1, 3, 8):
        run = FakeRun(rows=rows, gate=True)
        with Session(run, timeout=WAIT) as s:
            hs = [s.submit(t, stream=True, voice="v" if i % 2 else None) for i, t in enumerate(texts)]
            plain = s.submit("p:9|q:21", voice="v")
            run.gate.set()
            for h, w in zip(hs, want):
                same(collect(h), w)
            kind, voice, segs = plain.result()
            assert kind == "whole" and voice == "v" and [int(w.numel()) for w in segs] == [9 * UP - TRIM, 21 * UP - TRIM]
        assert ("p:9", "v", 0) in run.submitted and ("q:21", "v", 1) in run.submitted      # a plain request: RNG stream = segment index
    # one vocoder call and one post-processing launch per tick, however many listeners have a piece due
    assert run.posts <= run.steps and run.vocodes <= 2 * run.steps


def test_a_finished_item_flushes_a_short_last_piece():
    got = None
    with Session(FakeRun(), timeout=WAIT) as s:
        got = collect(s.submit("c:14", stream=True))
    assert [int(p.numel()) for p in got] == [12 * UP - TRIM, 2 * UP]
    assert float(got[0][0]) >= 10000.0 and float(got[1][0]) < 10000.0                   # the first piece's flags once
    same(got, alone("c:14"))
    with Session(FakeRun(), timeout=WAIT) as s:                                          # an end right behind a cut: one middle piece
        got = collect(s.submit("d:49:e12", stream=True))
    assert len(got) == 1
    same(got, alone("d:49:e12"))


def test_a_silent_first_chunk_is_measured_again_and_dropped():
    with Session(FakeRun(), timeout=WAIT) as s:
        got = collect(s.submit("e:60:silent", stream=True))
    assert [int(p.numel()) for p in got] == [36 * UP, 12 * UP] and float(got[0].max()) >= 10000.0      # the second piece is the first
    same(got, alone("e:60:silent"))


def test_segments_of_a_streaming_request_come_in_order_with_stream_zero():
    run = FakeRun(rows=4)
    with Session(run, timeout=WAIT) as s:
        got = collect(s.submit("x:30|y:5|z:13", stream=True, voice="v"))
    same(got, alone("x:30", "v") + alone("y:5", "v") + alone("z:13", "v"))
    assert [i for _, _, i in run.submitted] == [0, 0, 0]


def test_submission_order_is_kept_within_a_voice():
    run = FakeRun(rows=1, gate=True)
    with Session(run, timeout=WAIT) as s:
        hs = [s.submit(f"t{k}:{5 + k}", voice="v" if k % 2 else None) for k in range(6)]
        run.gate.set()
        for h in hs:
            assert h.result()[0] == "whole"
    assert run.placed == [f"t{k}:{5 + k}" for k in range(6)]


def test_cancel_before_placement_mid_stream_and_after_the_end():
    run = FakeRun(rows=1, gate=True, pause_at=4)
    with Session(run, timeout=WAIT) as s:
        a = s.submit("a:100", stream=True)
        b = s.submit("b:20")                            # waits behind a: cancelled before it has a row
        c = s.submit("c:7")
        b.cancel()
        run.gate.set()
        it = iter(a)
        first = next(it)                                # (12 frames = three steps; the fourth waits)
        same([first], alone("a:100")[:1])
        assert run.paused.wait(WAIT)
        a.cancel()                                      # mid-stream: iteration ends, the row goes to c
        run.gate.set()
        assert list(it) == []
        with pytest.raises(RequestCancelled):
            a.result()
        with pytest.raises(RequestCancelled):
            b.result()
        assert c.result()[0] == "whole"
        c.cancel()                                      # after the end: nothing happens
        d = s.submit("d:3")
        assert d.result()[0] == "whole" and c.result()[0] == "whole"
    assert "b:20" not in run.placed and "a:100" in run.cancelled and "c:7" not in run.cancelled


def test_an_exception_in_the_run_reaches_every_pending_handle():
    run = FakeRun(rows=1, gate=True, fail_at=3)
    s = Session(run, timeout=WAIT)
    try:
        hs = [s.submit("a:100", stream=True), s.submit("b:5"), s.submit("c:5", stream=True)]
        run.gate.set()
        for h in hs:
            with pytest.raises(RuntimeError, match="boom"):
                h.result()
        with pytest.raises(RuntimeError, match="boom"):
            collect(hs[2])
        with pytest.raises(SessionClosed):
            s.submit("d:5")
    finally:
        s.close()
    assert run.closes == 1


def test_a_refused_request_fails_alone():
    with Session(FakeRun(), timeout=WAIT) as s:
        bad, empty, good = s.submit("bad:5"), s.submit(""), s.submit("g:5")
        with pytest.raises(ValueError, match="refused"):
            bad.result()
        with pytest.raises(ValueError):
            empty.result()
        assert good.result()[0] == "whole"


def test_close_with_pending_requests_cancels_them():
    run = FakeRun(rows=1, gate=True, pause_at=2)
    s = Session(run, timeout=WAIT)
    hs = [s.submit("a:1000", stream=True), s.submit("b:5")]
    run.gate.set()
    assert run.paused.wait(WAIT)                        # a decodes, b waits for its row; the worker is inside a step
    closer = threading.Thread(target=s.close)
    closer.start()
    assert s.closing.wait(WAIT)
    run.gate.set()
    closer.join(WAIT)
    assert not closer.is_alive()
    for h in hs:
        with pytest.raises(SessionClosed):
            h.result()
    with pytest.raises(SessionClosed):
        collect(hs[0])
    with pytest.raises(SessionClosed):
        s.submit("c:5")
    assert run.closes == 1
    s.close()                                           # twice: nothing more
    assert run.closes == 1


def test_a_spent_horizon_is_drained_and_reopened_without_losing_a_request():
    texts = [f"h{k}:{20 + k}" for k in range(7)]
    run = FakeRun(rows=2, horizon=60, gate=True)
    with Session(run, timeout=WAIT) as s:
        hs = [s.submit(t, stream=True) for t in texts]
        run.gate.set()
        for h, t in zip(hs, texts):
            same(collect(h), alone(t))
        assert s.reopened >= 2 and run.opens == s.reopened + 1
        never = s.submit("n:100")                       # more than a whole horizon: refused for good, nobody else disturbed
        with pytest.raises(RuntimeError, match="horizon"):
            never.result()
        assert s.submit("o:10").result()[0] == "whole"
    assert run.placed[:7] == texts


def test_a_wait_that_runs_out_is_an_error():
    run = FakeRun(gate=True)
    s = Session(run, timeout=WAIT)
    try:
        h = s.submit("a:5", stream=True)
        with pytest.raises(TimeoutError):
            h.result(timeout=0.0)
        assert isinstance(h, Handle) and not h.done()
        run.gate.set()
        assert h.result() is None and h.done()
        with pytest.raises(TypeError):
            iter(s.submit("b:5")).__next__()
    finally:
        s.close()
