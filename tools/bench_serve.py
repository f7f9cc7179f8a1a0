#!/usr/bin/env python
"""Serving benchmark: one seeded arrival schedule, served twice.

  session     every request is submitted to ONE serving session (MI355XQwenTTS.serve) at its arrival time and streams from there
  sequential  the way it had to be done before sessions: stream() calls one after the other, in arrival order, each starting when
              the one before it has ended (or at its own arrival time, whichever is later)

Per request: time to first audio (arrival -> first piece) and completion time (arrival -> last piece).  In total: audio seconds per
wall second, and for the session the mean number of busy decode rows (rt_generate_stats: frames kept / frames run).

    python tools/bench_serve.py --model 1.7b --rows 32 --requests 36 --rate 6

Prints one line per request on stderr and ONE JSON line on stdout.  Synthetic weights (seeded), texts from bench.py's corpus."""
import argparse
import json
import os
import statistics
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def schedule(n, rate, seed, n_voices):
    """n requests: (arrival time in s, text, voice index) - exponential gaps of mean 1 / rate, texts of 6 .. 24 words"""
    import numpy as np
    from bench import sentences
    rng = np.random.default_rng(seed)
    gaps = rng.exponential(1.0 / rate, n)
    gaps[0] = 0.0
    voices = rng.integers(0, n_voices, n)
    return [(float(t), s, int(v)) for t, s, v in zip(np.cumsum(gaps), sentences(n, (6, 24), seed), voices)]


def wait_until(t0, at):
    d = t0 + at - time.perf_counter()
    if d > 0:
        time.sleep(d)


def audio_seconds(pieces):
    return sum(p.duration_sec for p in pieces)


def run_session(tts, sched, names, args):
    rec = [None] * len(sched)

    def listen(i, h, t0, at):
        first, pieces = None, []
        for p in h:
            if first is None:
                first = time.perf_counter() - t0 - at
            pieces.append(p)
        rec[i] = dict(ttfa=first, done=time.perf_counter() - t0 - at, audio=audio_seconds(pieces), pieces=len(pieces))
    with tts.serve(rows=args.rows, voices=[n for n in names if n], stream_chunk_frames=args.first, stream_next_chunk_frames=args.next,
                   horizon=args.horizon, timeout=args.timeout) as s:
        threads = []
        t0 = time.perf_counter()
        for i, (at, text, v) in enumerate(sched):
            wait_until(t0, at)
            h = s.submit(text, voice=names[v], stream=True)
            th = threading.Thread(target=listen, args=(i, h, t0, at), daemon=True)
            th.start()
            threads.append(th)
        for th in threads:
            th.join(args.timeout)
        wall = time.perf_counter() - t0
        run = s.run
    kept = sum(st["frames_kept"] for st in run.stats)
    launched = sum(st["frames_run"] for st in run.stats)
    return rec, wall, dict(mean_busy_rows=kept / max(1, launched), frames_run=launched, rows=args.rows, runs=len(run.stats))


def run_sequential(tts, sched, names, args):
    before = tts.stream_chunk_frames, tts.stream_next_chunk_frames
    tts.stream_chunk_frames, tts.stream_next_chunk_frames = args.first, args.next
    rec = []
    t0 = time.perf_counter()
    for at, text, v in sched:
        wait_until(t0, at)
        first, pieces = None, []
        for p in tts.stream(text):                       # (sub-segment streaming speaks with the constructor's voice only)
            if first is None:
                first = time.perf_counter() - t0 - at
            pieces.append(p)
        rec.append(dict(ttfa=first, done=time.perf_counter() - t0 - at, audio=audio_seconds(pieces), pieces=len(pieces)))
    tts.stream_chunk_frames, tts.stream_next_chunk_frames = before
    return rec, time.perf_counter() - t0, {}


def frame_cost(tts, args, frames=44, passes=5):
    """ms per decode frame with every row busy and ONE voice: the closed-list single-voice run against an open run that declares that
    voice (the block-table form).  Each pass: begin / open, one step that places the items, then `frames` timed frames; median."""
    from bench import sentences
    eng = tts._load_engine()
    with tts._lock:
        tts._ensure_voice(eng)
    nm, rows = eng.model, args.rows
    ids = [eng.tokenizer.encode(t) for t in sentences(rows, 10, args.seed)]
    kw = dict(talker=eng.params.talker(), predictor=eng.params.predictor(), seed=args.seed)
    budget = [2 * frames + 8] * rows

    def timed():
        nm.generate_step(1)
        eng.ctx.synchronize()
        t0 = time.perf_counter()
        nm.generate_step(frames)
        eng.ctx.synchronize()
        dt = time.perf_counter() - t0
        nm.generate_end()
        return 1e3 * dt / frames
    closed, opened = [], []
    for _ in range(passes + 1):                          # (the first pass warms both forms up: graphs)
        nm.generate_begin(ids, budget, item_ids=list(range(rows)), **kw)
        closed.append(timed())
        nm.generate_open(rows, max(len(i) for i in ids), budget[0], 16 * budget[0], [0], first=[(i, budget[0], k, 0) for k, i in enumerate(ids)], **kw)
        opened.append(timed())
    c, o = statistics.median(closed[1:]), statistics.median(opened[1:])
    return dict(rows=rows, frames=frames, closed_ms=[round(v, 4) for v in closed[1:]], open_ms=[round(v, 4) for v in opened[1:]],
                closed_median_ms=round(c, 4), open_median_ms=round(o, 4), open_over_closed=round(o / c, 4))


def summary(rec, wall, extra):
    ttfa = [r["ttfa"] for r in rec if r and r["ttfa"] is not None]
    audio = sum(r["audio"] for r in rec if r)
    out = dict(requests=len(rec), served=len(ttfa), ttfa_median_s=round(statistics.median(ttfa), 4), ttfa_worst_s=round(max(ttfa), 4),
               done_median_s=round(statistics.median(r["done"] for r in rec if r), 4), audio_s=round(audio, 2), wall_s=round(wall, 3),
               audio_s_per_s=round(audio / wall, 2))
    out.update({k: (round(v, 2) if isinstance(v, float) else v) for k, v in extra.items()})
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--model", default="1.7b", help="config preset: 1.7b | 0.6b | small | tiny")
    ap.add_argument("--rows", type=int, default=32)
    ap.add_argument("--requests", type=int, default=36)
    ap.add_argument("--rate", type=float, default=6.0, help="mean arrivals per second")
    ap.add_argument("--seed", type=int, default=789)
    ap.add_argument("--voices", type=int, default=1, help="session mode: voices the requests are dealt over (1: the constructor's; the "
                                                          "sequential mode always speaks with that one)")
    ap.add_argument("--first", type=int, default=12)
    ap.add_argument("--next", type=int, default=36)
    ap.add_argument("--horizon", type=int, default=4096)
    ap.add_argument("--timeout", type=float, default=300.0)
    ap.add_argument("--mode", default="both", choices=["both", "session", "sequential", "none"])
    ap.add_argument("--frame-cost", action="store_true", help="also: ms per frame of an open run with one declared voice against the "
                                                              "closed single-voice run, every row busy")
    args = ap.parse_args()
    os.environ.setdefault("RHO_TTS_AMD_SYNTHETIC", "1")         # seeded synthetic weights of the named architecture
    from rho_tts_amd.provider import MI355XQwenTTS
    speakers = ["Ryan", "Vivian"]
    tts = MI355XQwenTTS(device="cuda", speaker="Vivian", model_path=f"x/CustomVoice-{args.model}", batch_size=args.rows, max_iterations=1,
                        max_voices=max(1, min(8, args.voices)))
    names = [None]
    for k in range(1, max(1, min(8, args.voices))):
        names.append(f"v{k}")
        tts.add_voice(names[-1], speaker=speakers[k % 2])
    sched = schedule(args.requests, args.rate, args.seed, len(names))
    out = dict(model=args.model, rows=args.rows, rate=args.rate, first=args.first, next=args.next, voices=len(names))
    try:
        if args.mode != "none":
            list(tts.stream(sched[0][1]))                # warm-up: engine, voice, graphs
        for mode, fn in (("session", run_session), ("sequential", run_sequential)):
            if args.mode not in ("both", mode):
                continue
            if mode == "session":
                with tts.serve(rows=args.rows, voices=[n for n in names if n], timeout=args.timeout) as s:      # warm-up: the open run's graphs
                    list(s.submit(sched[0][1], stream=True))
            rec, wall, extra = fn(tts, sched, names, args)
            for i, (r, (at, text, v)) in enumerate(zip(rec, sched)):
                if r is None or r["ttfa"] is None:
                    print(f"{mode:10s} #{i:02d} t={at:7.3f}s voice {v} words {len(text.split()):2d}: not served", file=sys.stderr, flush=True)
                    continue
                print(f"{mode:10s} #{i:02d} t={at:7.3f}s voice {v} words {len(text.split()):2d}: first audio {r['ttfa']:.3f}s, done {r['done']:.3f}s, "
                      f"{r['audio']:.2f}s of audio in {r['pieces']} pieces", file=sys.stderr, flush=True)
            out[mode] = summary(rec, wall, extra)
        if args.frame_cost:
            out["frame_cost"] = frame_cost(tts, args)
    finally:
        tts.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
