#!/usr/bin/env python3
"""Drift features of one validation chunk: the per-clip loop (HandcraftedFeatures.__call__: one native call per clip, difference
function off the GPU, pYIN's back half on the host, one host synchronisation per clip) against HandcraftedFeatures.batch (one native
call, one launch per stage for the whole chunk, pYIN's back half in HIP kernels, one synchronisation per chunk).  Both go through the
same native path and the same workspace set of one handle, alternately - so the loop also exercises a one-clip call after a 32-clip
one.  32 synthetic voiced clips of 4 s at 24 kHz, in HBM; five alternating pairs in one process; both outputs are compared before
anything is timed.
    python tools/bench_features.py [n_clips] [seconds]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from rho_tts_amd import _native
from rho_tts_amd import features as PF

N = int(sys.argv[1]) if len(sys.argv) > 1 else 32
SECONDS = float(sys.argv[2]) if len(sys.argv) > 2 else 4.0
SR, PAIRS = 24000, 5


def voiced(seconds, f0, seed):
    t = np.arange(int(seconds * SR)) / SR
    x = 0.3 * sum(np.sin(2 * np.pi * f0 * (k + 1) * t) / (k + 1) for k in range(5)) * (0.6 + 0.4 * np.sin(2 * np.pi * 3 * t))
    x[: int(0.1 * SR)] = 0.0
    return (x + 1e-3 * np.random.default_rng(seed).standard_normal(x.shape[0])).astype(np.float32)


ctx = _native.Context(0)
ex = PF.HandcraftedFeatures(ctx)
clips = [torch.from_numpy(voiced(SECONDS, 110.0 + 7.0 * c, c)).cuda() for c in range(N)]
torch.cuda.synchronize()
per_clip = lambda: np.stack([ex(x, SR) for x in clips])      # noqa: E731
batched = lambda: ex.batch(clips, SR)                        # noqa: E731
a, b = per_clip(), batched()                                 # warm-up of both paths, and the check that they compute the same
frames = len(ex.f0_states(clips[:1], SR)[0])
print(f"{N} clips of {SECONDS:g} s at {SR} Hz, {frames} pitch frames per clip; outputs equal: {bool(np.array_equal(a, b))}"
      f" (max |difference| {float(np.abs(a - b).max()):.3g})", flush=True)
t_clip, t_batch = [], []
for p in range(PAIRS):
    t0 = time.perf_counter()
    per_clip()
    t1 = time.perf_counter()
    batched()
    t2 = time.perf_counter()
    t_clip.append((t1 - t0) * 1e3)
    t_batch.append((t2 - t1) * 1e3)
    print(f"pair {p + 1}: per-clip loop {t_clip[-1]:9.2f} ms   batch() {t_batch[-1]:8.2f} ms   ratio {t_clip[-1] / t_batch[-1]:6.1f}"
          f"   batch faster: {t_batch[-1] < t_clip[-1]}", flush=True)
mc, mb = sorted(t_clip)[PAIRS // 2], sorted(t_batch)[PAIRS // 2]
print(f"median: per-clip loop {mc:.2f} ms ({mc / N:.2f} ms per clip)   batch() {mb:.2f} ms ({mb / N:.3f} ms per clip)   ratio {mc / mb:.1f}")
print(f"batch() faster in every pair: {all(y < x for x, y in zip(t_clip, t_batch))}")
ex.close()
ctx.close()
