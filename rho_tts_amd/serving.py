"""Serving sessions: requests join a decode batch in flight and stream (rt_generate_open / _submit / _cancel_item underneath).

A ``Session`` owns ONE worker thread that drives one open run.  Callers ``submit`` texts from any thread and get a ``Handle``; the
worker admits the segments of every request to the run, steps it ``every`` frames at a time (the hand-over cadence), and hands out

  - for a ``stream=True`` request the pieces of every segment, cut where ITS OWN frame count reaches ``first_chunk``, then
    ``+ chunk`` - counted from the segment's first frame, not from the tick it arrived in - vocoded with the codec's left context and
    levelled / trimmed / faded by rt_stream_chunks.  A tick makes ONE vocoder call and ONE post-processing launch for all listeners.
  - for a plain request one result: its segments vocoded, joined and post-processed as ``generate`` does with ``max_iterations == 1``.

Because the cuts are per item and an item's codes are what it gets alone, a request's audio does not depend on who else is connected.

The scheduler is written against a small run interface (``Session.__init__``) so that the cut logic, ordering, cancellation, error
delivery and shutdown are tested on the CPU with a fake run (tests/test_serving_cpu.py); ``EngineRun`` is the one over an Engine."""
from __future__ import annotations

import collections
import threading
from typing import Callable, Deque, List, Optional, Sequence

import torch


class HorizonSpent(RuntimeError):
    """``run.submit``: the open run's frame counter cannot hold the item.  The session stops admitting, drains, reopens, goes on."""


class SessionClosed(RuntimeError):
    """The session was closed (or broke) while the request was pending."""


class RequestCancelled(RuntimeError):
    """``Handle.cancel`` was called before the request had finished."""


_END = object()


class _Segment:
    __slots__ = ("req", "index", "text", "item", "epoch", "frames", "sent", "emitted", "started", "state", "codes", "done", "pieces")

    def __init__(self, req, index, text):
        self.req, self.index, self.text = req, index, text
        self.item: Optional[int] = None                        # its index in the run of `epoch`; None: still waiting to be admitted
        self.epoch = -1
        self.frames = 0                                        # its frame budget (run.submit tells)
        self.sent = 0                                          # frames handed to the vocoder so far
        self.emitted = 0                                       # samples cut off so far = absolute position of the next one
        self.started = False                                   # audible audio of this segment has been handed out
        self.state = [0.0, 1.0]                                # (dc, gain) carried from its first audible piece
        self.codes: Optional[torch.Tensor] = None              # every frame decoded so far
        self.done = False
        self.pieces: List[object] = []                         # processed pieces not yet released (segments are released in order)


class Handle:
    """One request of a session.  ``result(timeout)``: the finished request (a ``GenerationResult``; ``None`` for a streaming one,
    whose audio is what iterating the handle yields).  Waits are bounded: ``TimeoutError`` when the time runs out."""

    def __init__(self, session, text, voice, stream, speed, pitch, timeout):
        self._session, self.text, self.voice, self.stream = session, text, voice, bool(stream)
        self.speed, self.pitch = float(speed), float(pitch)
        self._timeout = timeout
        self._cond = threading.Condition()
        self._queue: Deque[object] = collections.deque()       # pieces of a streaming request, then _END
        self._done = False
        self._result = None
        self._error: Optional[BaseException] = None
        self.segments: List[_Segment] = []
        self._released = 0                                     # segments whose pieces have all been put on the queue

    # ---- the worker's side
    def _put(self, piece) -> None:
        with self._cond:
            self._queue.append(piece)
            self._cond.notify_all()

    def _finish(self, result=None, error: Optional[BaseException] = None) -> None:
        with self._cond:
            if self._done:
                return
            self._done, self._result, self._error = True, result, error
            self._queue.append(_END)
            self._cond.notify_all()

    # ---- the caller's side
    def done(self) -> bool:
        with self._cond:
            return self._done

    def cancel(self) -> None:
        """End the request: its rows are free at the run's next look.  ``result`` raises ``RequestCancelled``; iteration stops."""
        self._session._cancel(self)

    def result(self, timeout: Optional[float] = None):
        timeout = self._timeout if timeout is None else timeout
        with self._cond:
            if not self._cond.wait_for(lambda: self._done, timeout):
                raise TimeoutError(f"the request did not finish within {timeout} s")
            if self._error is not None:
                raise self._error
            return self._result

    def __iter__(self):
        if not self.stream:
            raise TypeError("only a stream=True request yields pieces; use result()")
        while True:
            with self._cond:
                if not self._cond.wait_for(lambda: len(self._queue) > 0, self._timeout):
                    raise TimeoutError(f"no piece within {self._timeout} s")
                piece = self._queue.popleft()
                if piece is _END:
                    self._queue.append(_END)                   # (a second iteration ends at once)
                    if self._error is not None and not isinstance(self._error, RequestCancelled):
                        raise self._error
                    return
            yield piece


def piece_is_last(finished: bool, total: int, cut: int, budget: int) -> bool:
    """Is the piece that ends at frame ``cut`` (or at ``total`` < cut) the item's last, AS A CALLER THAT STEPS THE ITEM ALONE SEES IT
    (Engine.stream_codes)?  Alone, the item is stepped exactly to the cut: it is known to have ended there only if it ended below the
    cut, or on it by spending its frame budget - an end-of-sequence frame right behind the cut has not been run yet, and the piece
    goes out as a middle one (the last one is then empty)."""
    return bool(finished) and (total < cut or (total == cut and total >= budget))


class Session:
    """The scheduler.  ``run`` offers
        every                                   frames per step (the hand-over cadence)
        open() / close()                        begin / end the open run (close may be called on a broken run)
        submit(text, voice, item_id) -> (item, frame budget)   raises HorizonSpent; any other exception fails the request
        step(n) -> all_done                     n more frames (none when nothing decodes)
        peek(item, first, n) -> (codes, finished)
        cancel(item)
        split(text) -> [segment texts]
        vocode([codes]) -> [raw wav]            one call for every piece of a tick ([left context + new frames] each)
        context(start) -> frames of left context for a piece that begins at frame `start`;  samples(frames) -> samples per frame run
        post([wav], [state], [(first, last)]) -> [wav]     one launch; states updated in place (gain 0: nothing measured)
        vocode_whole([codes]) -> [raw wav]      whole segments (chunked as the codec decoder chunks them)
        finish([[wav]], [request]) -> [result]  join + post-processing + result of plain requests
        wrap(wav, request) -> piece             the result object of one streamed piece
    """

    def __init__(self, run, first_chunk: int = 12, chunk: int = 36, timeout: float = 120.0, on_close: Optional[Callable[[], None]] = None):
        if int(first_chunk) < 1 or int(chunk) < 1:
            raise ValueError("chunk sizes are at least one frame")
        self.run, self.first_chunk, self.chunk, self.timeout = run, int(first_chunk), int(chunk), float(timeout)
        self._on_close = on_close
        self._lock = threading.Condition()
        self._inbox: Deque[Handle] = collections.deque()       # submitted, not yet seen by the worker
        self._cancels: Deque[Handle] = collections.deque()
        self._waiting: Deque[_Segment] = collections.deque()   # segments not yet admitted to the run, in submission order
        self._live: List[_Segment] = []                        # admitted, not finished
        self._requests: List[Handle] = []                      # every request that has not finished
        self.closing = threading.Event()                       # close() has been called: the worker stops at its next look
        self._error: Optional[BaseException] = None
        self._epoch = 0
        self._draining = False
        self._fresh = True                                     # the run has not been stepped since it was opened
        self.reopened = 0
        self.ticks = 0
        run.open()
        self._worker = threading.Thread(target=self._work, name="rho-tts-session", daemon=True)
        self._worker.start()

    # ------------------------------------------------------------------ the callers' side (any thread)
    def submit(self, text: str, voice: Optional[str] = None, stream: bool = False, speed: float = 1.0, pitch_semitones: float = 0.0) -> Handle:
        h = Handle(self, text, voice, stream, speed, pitch_semitones, self.timeout)
        with self._lock:
            if self.closing.is_set():
                raise SessionClosed("the session is closed")
            if self._error is not None:
                raise SessionClosed(f"the session broke: {self._error}")
            self._inbox.append(h)
            self._lock.notify_all()
        return h

    def _cancel(self, h: Handle) -> None:
        with self._lock:
            self._cancels.append(h)
            self._lock.notify_all()

    def is_worker(self) -> bool:
        return threading.current_thread() is self._worker

    def close(self) -> None:
        """Stop the worker, cancel what is pending (those handles raise ``SessionClosed``) and end the run."""
        with self._lock:
            if self.closing.is_set():
                return
            self.closing.set()
            self._lock.notify_all()
        self._worker.join(self.timeout)
        stuck = self._worker.is_alive()
        self._fail_all(SessionClosed("the session was closed with the request pending"))
        try:
            if not stuck:
                self.run.close()
        finally:
            if self._on_close is not None:
                self._on_close()
        if stuck:
            raise TimeoutError(f"the session's worker did not stop within {self.timeout} s")

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    # ------------------------------------------------------------------ the worker
    def _fail_all(self, error: BaseException) -> None:
        with self._lock:
            pending = list(self._requests) + list(self._inbox)
            self._requests, self._live = [], []
            self._inbox.clear()
            self._waiting.clear()
        for h in pending:
            h._finish(error=error)

    def _work(self) -> None:
        try:
            while True:
                with self._lock:
                    while not (self.closing.is_set() or self._inbox or self._cancels or self._live or self._waiting):
                        self._lock.wait(0.5)                   # (idle: nothing to decode; woken by submit / cancel / close)
                    if self.closing.is_set():
                        return
                    inbox, self._inbox = list(self._inbox), collections.deque()
                    cancels, self._cancels = list(self._cancels), collections.deque()
                self._take(inbox)
                self._apply_cancels(cancels)
                self._admit()
                if self._live:
                    self._tick()
                elif self._waiting and not self._draining:
                    raise RuntimeError("a waiting segment was not admitted to an empty run")
                if self._draining and not self._live:          # the horizon was spent and the run has drained: a fresh run for the queue
                    self.run.close()
                    self.run.open()
                    self._epoch += 1
                    self.reopened += 1
                    self._draining = False
                    self._fresh = True
        except BaseException as e:  # noqa: BLE001  (whatever broke the run reaches every pending handle)
            with self._lock:
                self._error = e
            self._fail_all(e)

    def _take(self, inbox: Sequence[Handle]) -> None:
        for h in inbox:
            try:
                texts = list(self.run.split(h.text))
                if not texts:
                    raise ValueError("the text has no segment to speak")
            except Exception as e:  # noqa: BLE001
                h._finish(error=e)
                continue
            h.segments = [_Segment(h, k, t) for k, t in enumerate(texts)]
            self._requests.append(h)
            self._waiting.extend(h.segments)

    def _drop(self, h: Handle, error: BaseException) -> None:
        """take every segment of the request out of the run and the queue, and end its handle"""
        for s in h.segments:
            if s.item is not None and not s.done and s.epoch == self._epoch:
                self.run.cancel(s.item)
            s.done = True
        self._live = [s for s in self._live if s.req is not h]
        self._waiting = collections.deque(s for s in self._waiting if s.req is not h)
        if h in self._requests:
            self._requests.remove(h)
        h._finish(error=error)

    def _apply_cancels(self, cancels: Sequence[Handle]) -> None:
        for h in cancels:
            if h in self._requests:                            # (after it has finished: nothing to do)
                self._drop(h, RequestCancelled("the request was cancelled"))

    def _admit(self) -> None:
        """waiting segments -> the run, in submission order (the run keeps that order within a voice)"""
        while self._waiting and not self._draining:
            s = self._waiting[0]
            try:
                # a plain request's segments take the RNG streams generate() gives them (the segment's index), a streaming one's all
                # stream 0, as stream() does
                s.item, s.frames = self.run.submit(s.text, s.req.voice, 0 if s.req.stream else s.index)
            except HorizonSpent as e:
                if self._fresh and not self._live:             # an empty run that has not decoded a frame cannot hold it: none ever will
                    self._drop(s.req, RuntimeError(f"length: the request does not fit the run's horizon ({e})"))
                    continue
                self._draining = True                          # stop admitting; what decodes drains, then a fresh run takes the queue
                return
            except Exception as e:  # noqa: BLE001  (refused: too long, unknown voice, ...: this request only)
                self._drop(s.req, e)
                continue
            s.epoch = self._epoch
            self._waiting.popleft()
            self._live.append(s)

    def _tick(self) -> None:
        run = self.run
        run.step(run.every)
        self._fresh = False
        self.ticks += 1
        due = []                                               # (segment, first frame of the decode, left context, last)
        for s in self._live:
            if not s.req.stream:                               # a plain request: the whole segment once it has ended
                if run.peek(s.item, 0, 0)[1]:
                    s.codes, s.done = run.peek(s.item, 0, s.frames)[0], True
                continue
            # a streaming one: a piece when ITS cut is reached or it has ended - peeked exactly up to the cut, so the pieces are those
            # of a caller that steps this item alone (one piece per segment and tick: the next joins the next tick's launches)
            cut = s.sent + (self.first_chunk if s.sent == 0 else self.chunk)
            codes, fin = run.peek(s.item, s.sent, cut - s.sent)
            have = s.sent + int(codes.shape[0])
            if have < cut and not fin:
                continue
            total = have + (int(run.peek(s.item, have, 1)[0].shape[0]) if fin and have == cut else 0)
            last = piece_is_last(fin, total, cut, s.frames)
            if codes.shape[0]:
                due.append((s, s.sent, run.context(s.sent), last))
                s.codes = codes if s.codes is None else torch.cat([s.codes, codes])
                s.sent = have
            s.done = last or (fin and total == have)           # (ended right behind a cut: the piece went out as a middle one)
        if due:
            raws = run.vocode([s.codes[start - ctx:] for s, start, ctx, _ in due])
            pieces, flags = [], []
            for (s, start, ctx, last), w in zip(due, raws):
                off = max(0, s.emitted - (start - ctx) * run.samples(1))
                w = w[off:]
                s.emitted += int(w.numel())
                pieces.append(w)
                flags.append((not s.started, last))
            states = [s.state for s, _, _, _ in due]
            outs = run.post(pieces, states, flags)
            for (s, _, _, _), raw, out in zip(due, pieces, outs):
                if not s.started and raw.numel():
                    if s.state[1] > 0.0:
                        s.started = True
                    else:                                      # lead-in silence: nothing measured, nothing to play - the next piece is
                        continue                               # the segment's first (gain, trim, fade-in)
                if out.numel():
                    s.pieces.append(run.wrap(out, s.req))
        self._live = [s for s in self._live if not s.done]
        # release: a streaming request's pieces go out in segment order; a request ends when every segment has
        whole = []
        for h in list(self._requests):
            if h.stream:
                while h._released < len(h.segments):
                    s = h.segments[h._released]
                    for p in s.pieces:
                        h._put(p)
                    s.pieces = []
                    if not s.done:
                        break
                    h._released += 1
                if h._released == len(h.segments):
                    self._requests.remove(h)
                    h._finish(None)
            elif all(s.done for s in h.segments):
                whole.append(h)
        if whole:
            segs = [s for h in whole for s in h.segments]
            wavs = run.vocode_whole([s.codes for s in segs])
            by_seg = dict(zip(map(id, segs), wavs))
            results = run.finish([[by_seg[id(s)] for s in h.segments] for h in whole], whole)
            for h, r in zip(whole, results):
                self._requests.remove(h)
                if isinstance(r, BaseException):
                    h._finish(error=r)
                else:
                    h._finish(r)


class EngineRun:
    """The run interface of ``Session`` over an ``Engine`` and the provider that owns it (MI355XQwenTTS.serve)."""

    def __init__(self, provider, eng, rows, voices, max_text_tokens, max_frames, horizon):
        self.p, self.eng = provider, eng
        self.every = eng.model.cadence()                       # the library's hand-over cadence: the worker steps by it
        self._open = dict(rows=rows, voices=voices, max_text_tokens=max_text_tokens, max_frames=max_frames, horizon=horizon)
        self.caps: dict = {}
        self.stats: List[dict] = []                            # rt_generate_stats of every run this session has closed
        self.params = provider._post_params(0)

    def open(self) -> None:
        self.caps = self.eng.open_run(seed=int(self.p.seed), **self._open)

    def close(self) -> None:
        self.eng.model.generate_end()
        self.stats.append(self.eng.model.generate_stats())

    def split(self, text: str) -> List[str]:
        return self.p._split_text_into_segments(self.p._apply_phonetic_mapping(text), self.p._compute_max_chars())

    def submit(self, text: str, voice: Optional[str], item_id: int):
        from ._native import LengthError
        try:
            return self.eng.submit(text, voice, item_id)
        except LengthError as e:                               # (Engine.submit has checked the positions: this is the horizon)
            raise HorizonSpent(str(e)) from e

    def step(self, n: int) -> bool:
        return self.eng.model.generate_step(n)[1]

    def peek(self, item: int, first: int, n: int):
        return self.eng.model.generate_peek(item, first, n)

    def cancel(self, item: int) -> None:
        self.eng.cancel(item)

    def context(self, start: int) -> int:
        lc = self.eng.cfg.codec.left_context_frames
        return lc if start - lc > 0 else start

    def samples(self, frames: int) -> int:
        return frames * self.eng.cfg.codec.total_upsample

    def vocode(self, codes: Sequence[torch.Tensor]) -> List[torch.Tensor]:
        out: List[torch.Tensor] = []
        for i0 in range(0, len(codes), self.eng.max_batch):    # (one call for a tick's pieces unless there are more than decode rows)
            out += self.eng.model.code2wav(list(codes[i0:i0 + self.eng.max_batch]))
        return out

    def post(self, wavs, states, flags) -> List[torch.Tensor]:
        ctx = self.eng.ctx
        return ctx.stream_chunks(self.params, wavs, states, [ctx.stream_flags(f, l) for f, l in flags])

    def vocode_whole(self, codes: Sequence[torch.Tensor]) -> List[torch.Tensor]:
        return self.eng.vocode(codes)

    def _result(self, audio, req, n_segments, decay_ratio=None):
        from .hostapi import GenerationResult
        if req.speed != 1.0 or req.pitch != 0.0:
            audio = self.p._apply_speed_pitch(audio, req.speed, req.pitch)
        n_samples = audio.shape[-1] if audio.dim() == 2 else audio.numel()
        return GenerationResult(audio=audio, sample_rate=self.p.sample_rate, duration_sec=n_samples / self.p.sample_rate,
                                segments_count=n_segments, format="wav", decay_ratio=decay_ratio)

    def finish(self, items, requests) -> list:
        """join -> loudness -> decay of every finished request in one launch: the ``max_iterations == 1`` tail of ``generate``"""
        out = []
        for (audio, ratio, _ok), segs, req in zip(self.p._finish_items(items), items, requests):
            try:
                out.append(self._result(audio, req, len(segs), ratio))
            except Exception as e:  # noqa: BLE001  (this request only)
                out.append(e)
        return out

    def wrap(self, wav, req):
        return self._result(wav, req, 1)
