#!/usr/bin/env python3
"""Device time of speed / pitch control (rt_speedpitch_apply) on a 10-s clip at 24 kHz: speed 1.1, +4 and +0.5 semitones, each alone.

The call only enqueues kernels, so it is timed with device events on the stream it runs on (the context is put on torch's current
stream for that): `--calls` calls between two events, `--reps` such windows after a warm-up, median and spread per call.  Beside it
the float64 host restatement the tests compare against (tests/speed_pitch_ref.py), timed with a host clock on the same box, and the
distance of the two results.  `--no-host` leaves the restatement out (for a run under `rocprofv3 --kernel-trace`, whose per-kernel
times `tools/summarize_trace.py` splits by stage).
usage: bench_speed_pitch.py [--seconds 10] [--calls 20] [--reps 5] [--no-host] [--only +4]"""
import argparse
import ctypes as C
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from rho_tts_amd import _native, speedpitch
from tests import speed_pitch_ref as R

SR = 24000
CASES = (("speed 1.1", 1.1, 0.0), ("+4 semitones", 1.0, 4.0), ("+0.5 semitone", 1.0, 0.5))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--only", default="", help="run the cases whose name contains this (e.g. '+4')")
    a = ap.parse_args()
    n = int(a.seconds * SR)
    t = np.arange(n) / SR
    x = (0.4 * np.sin(2 * np.pi * 180.0 * t) * (0.6 + 0.4 * np.sin(2 * np.pi * 3.0 * t)) + 0.15 * np.sin(2 * np.pi * 1310.0 * t + 0.3) +
         0.05 * np.random.default_rng(789).standard_normal(n)).astype(np.float32)
    ctx = _native.Context(0)
    stream = torch.cuda.Stream()                               # (not the default stream: its handle is NULL, which rt_set_stream reads as "own")
    torch.cuda.set_stream(stream)
    ctx.set_stream(stream.cuda_stream)                         # torch's events bracket the context's work
    sp = speedpitch.SpeedPitch(ctx)
    d_x = torch.from_numpy(x).cuda()
    torch.cuda.synchronize()
    print(f"{a.seconds:g}-s clip at {SR} Hz ({n} samples); {a.calls} calls per window, {a.reps} windows", flush=True)
    for name, speed, steps in CASES:
        if a.only not in name:
            continue
        p =speedpitch.plan(n, SR, speed, steps)
        out = torch.empty(p.n_result, dtype=torch.float32, device="cuda")

        def call():
            ctx.check(sp.lib.rt_speedpitch_apply(sp.handle, C.c_void_p(d_x.data_ptr()), n, C.byref(p), C.c_void_p(out.data_ptr()), out.numel()), "apply")

        for _ in range(3):
            call()
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.calls):
                call()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1) / a.calls)
        ms.sort()
        terms = f"{p.s_o}:{p.s_n} width {p.s_width}" if speed != 1.0 else f"{p.nf} -> {p.n_out} frames, {p.p_o}:{p.p_n} width {p.p_width}"
        line = f"{name:14s} ({terms}) -> {p.n_result} samples: device {ms[len(ms) // 2]:.3f} ms per call (min {ms[0]:.3f}, max {ms[-1]:.3f})"
        if not a.no_host:
            t0 = time.perf_counter()
            ref = R.apply_speed_pitch(x.astype(np.float64), SR, speed, steps)
            host_ms = (time.perf_counter() - t0) * 1e3
            err = float(np.abs(out.cpu().numpy().astype(np.float64) - ref).max())
            line += f"; float64 host restatement {host_ms:.0f} ms; max|gpu - host| {err:.3g}"
        print(line, flush=True)
    sp.close()
    ctx.close()


if __name__ == "__main__":
    main()
