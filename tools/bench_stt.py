#!/usr/bin/env python3
"""Transcription of one validation chunk: the per-clip loop (NativeSTT.transcribe_ids per clip: front end, encoder and decoder
launched for one clip, one host synchronisation per generated token) against NativeSTT.transcribe_ids_batch (one native call: the
windows of all clips are the rows of every launch, one synchronisation per decode step for the chunk).  Whisper-tiny dimensions on
seeded weights, 32 synthetic voiced clips of 4 s at 24 kHz in HBM, max_new_tokens 16; five alternating pairs in one process; the
ids of both paths are compared before anything is timed.
    python tools/bench_stt.py [n_clips] [seconds] [max_new_tokens] [--once]
--once: one batched call and nothing else after the model is loaded (the run to take a kernel trace of)."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from rho_tts_amd import _native
from rho_tts_amd import stt as S

ARGS = [a for a in sys.argv[1:] if not a.startswith("--")]
ONCE = "--once" in sys.argv[1:]
N = int(ARGS[0]) if len(ARGS) > 0 else 32
SECONDS = float(ARGS[1]) if len(ARGS) > 1 else 4.0
MAX_NEW = int(ARGS[2]) if len(ARGS) > 2 else 16
SR, PAIRS = 24000, 5


def voiced(seconds, f0, seed):
    t = np.arange(int(seconds * SR)) / SR
    x = 0.3 * sum(np.sin(2 * np.pi * f0 * (k + 1) * t) / (k + 1) for k in range(5)) * (0.6 + 0.4 * np.sin(2 * np.pi * 3 * t))
    x[: int(0.1 * SR)] = 0.0
    return (x + 1e-3 * np.random.default_rng(seed).standard_normal(x.shape[0])).astype(np.float32)


if not torch.cuda.is_available():
    sys.exit("bench_stt.py measures on the GPU; there is none here")
ctx = _native.Context(0)
cfg = S.SttConfig(max_new_tokens=MAX_NEW)
nat = S.NativeSTT(ctx, cfg, S.synthetic_state(cfg, 789, device="cuda"))
clips = [torch.from_numpy(voiced(SECONDS, 110.0 + 7.0 * c, c)).cuda() for c in range(N)]
windows = sum(nat.windows(x.numel(), SR) for x in clips)
torch.cuda.synchronize()
per_clip = lambda: [nat.transcribe_ids(x, SR) for x in clips]      # noqa: E731
batched = lambda: nat.transcribe_ids_batch(clips, SR)              # noqa: E731
if ONCE:
    ids = batched()
    print(f"one batched call: {N} clips, {windows} windows, {sum(map(len, ids))} ids")
    nat.close()
    ctx.close()
    sys.exit(0)
free0 = torch.cuda.mem_get_info()[0]
b = batched()                                                      # warm-up of both paths, and the check that they compute the same
free1 = torch.cuda.mem_get_info()[0]
a = per_clip()
if a != b:
    sys.exit(f"the batched ids differ from the per-clip ids: {[i for i in range(N) if a[i] != b[i]]}")
group = min(windows, 32)
print(f"{N} clips of {SECONDS:g} s at {SR} Hz, {windows} windows, max_new_tokens {MAX_NEW}; ids equal: True ({sum(map(len, a))} ids, "
      f"{min(map(len, a))} .. {max(map(len, a))} per clip)", flush=True)
print(f"device memory taken by the first batched call: {(free0 - free1) / 2**20:.0f} MiB = {(free0 - free1) / group / 1e6:.1f} MB per window "
      f"of a group of {group}", flush=True)
t_clip, t_batch = [], []
for p in range(PAIRS):
    t0 = time.perf_counter()
    per_clip()
    t1 = time.perf_counter()
    batched()
    t2 = time.perf_counter()
    t_clip.append((t1 - t0) * 1e3)
    t_batch.append((t2 - t1) * 1e3)
    print(f"pair {p + 1}: per-clip loop {t_clip[-1]:9.2f} ms   batch {t_batch[-1]:8.2f} ms   ratio {t_clip[-1] / t_batch[-1]:6.1f}"
          f"   batch faster: {t_batch[-1] < t_clip[-1]}", flush=True)
mc, mb = sorted(t_clip)[PAIRS // 2], sorted(t_batch)[PAIRS // 2]
print(f"median: per-clip loop {mc:.2f} ms ({mc / N:.2f} ms per clip)   batch {mb:.2f} ms ({mb / N:.3f} ms per clip)   ratio {mc / mb:.1f}")
print(f"batch faster in every pair: {all(y < x for x, y in zip(t_clip, t_batch))}")
nat.close()
ctx.close()
