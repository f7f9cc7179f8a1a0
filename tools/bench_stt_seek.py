#!/usr/bin/env python3
"""Clips longer than one window: the seek call (NativeSTT.transcribe_ids_seek: timestamp tokens, the next window at the last closed
pair) against the fixed-cut call (NativeSTT.transcribe_ids_ex) of the same build, on the same clips in the same process.  Whisper-tiny
dimensions on seeded weights, 32 synthetic voiced clips of 45 s at 24 kHz in HBM, max_new_tokens 16, beam widths 1 and 5; alternating
pairs.  Both calls run the probe pass (no-speech probabilities asked for).  The fixed-cut call decodes ceil(45 / 30) = 2 windows per
clip in one sweep of groups; the seek call decodes one window per unfinished clip per round, so a clip's windows are serial, and it
decodes as many windows as its timestamps ask for.
    python tools/bench_stt_seek.py [n_clips] [seconds] [max_new_tokens] [--pairs N]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from rho_tts_amd import _native
from rho_tts_amd import stt as S

argv = sys.argv[1:]
PAIRS = int(argv[argv.index("--pairs") + 1]) if "--pairs" in argv else 5
ARGS = [a for i, a in enumerate(argv) if not a.startswith("--") and (i == 0 or argv[i - 1] != "--pairs")]
N = int(ARGS[0]) if len(ARGS) > 0 else 32
SECONDS = float(ARGS[1]) if len(ARGS) > 1 else 45.0
MAX_NEW = int(ARGS[2]) if len(ARGS) > 2 else 16
SR = 24000


def voiced(seconds, f0, seed):
    t = np.arange(int(seconds * SR)) / SR
    x = 0.3 * sum(np.sin(2 * np.pi * f0 * (k + 1) * t) / (k + 1) for k in range(5)) * (0.6 + 0.4 * np.sin(2 * np.pi * 3 * t))
    x[: int(0.1 * SR)] = 0.0
    return (x + 1e-3 * np.random.default_rng(seed).standard_normal(x.shape[0])).astype(np.float32)


if not torch.cuda.is_available():
    sys.exit("bench_stt_seek.py measures on the GPU; there is none here")
ctx = _native.Context(0)
cfg = S.SttConfig(max_new_tokens=MAX_NEW, timestamp_begin=50364)
nat = S.NativeSTT(ctx, cfg, S.synthetic_state(cfg, 789, device="cuda"))
clips = [torch.from_numpy(voiced(SECONDS, 110.0 + 7.0 * c, c)).cuda() for c in range(N)]
torch.cuda.synchronize()
print(f"{N} clips of {SECONDS:g} s at {SR} Hz, Whisper-tiny dimensions, seeded weights, max_new_tokens {MAX_NEW}, max_initial_timestamp_index "
      f"{cfg.max_initial_timestamp_index}; {PAIRS} alternating pairs per width", flush=True)
for beam in (1, 5):
    fixed = lambda: nat.transcribe_ids_ex(clips, SR, beam)             # noqa: E731
    seek = lambda: nat.transcribe_ids_seek(clips, SR, beam)            # noqa: E731
    f, k = fixed(), seek()                                              # (the first calls allocate the groups' buffers)
    w_fixed, w_seek = sum(len(c.windows) for c in f), sum(len(c.windows) for c in k)
    rounds = max(len(c.windows) for c in k)
    per_group = 32 // beam
    groups_fixed = -(-w_fixed // per_group)
    groups_seek = sum(-(-sum(1 for c in k if len(c.windows) > r) // per_group) for r in range(rounds))
    adv = [w.advance for c in k for w in c.windows]
    print(f"beam {beam}: fixed cuts decode {w_fixed} windows in {groups_fixed} groups; seek decodes {w_seek} windows in {rounds} rounds = {groups_seek} groups "
          f"(windows per clip {min(len(c.windows) for c in k)} .. {rounds}; advance {min(adv)} .. {max(adv)} ticks of a 1500-tick window; "
          f"segments per clip {min(len(c.segments) for c in k)} .. {max(len(c.segments) for c in k)}; "
          f"{sum(1 for a, b in zip(f, k) if a.ids != b.ids)} of {N} clips have other ids than with fixed cuts)", flush=True)
    t_f, t_k = [], []
    for p in range(PAIRS):
        t0 = time.perf_counter()
        fixed()
        t1 = time.perf_counter()
        seek()
        t2 = time.perf_counter()
        t_f.append((t1 - t0) * 1e3)
        t_k.append((t2 - t1) * 1e3)
        print(f"  pair {p + 1}: fixed cuts {t_f[-1]:9.2f} ms   seek {t_k[-1]:9.2f} ms   ratio {t_k[-1] / t_f[-1]:5.2f}", flush=True)
    mf, mk = sorted(t_f)[PAIRS // 2], sorted(t_k)[PAIRS // 2]
    print(f"  median: fixed cuts {mf:.2f} ms ({mf / w_fixed:.3f} ms per window)   seek {mk:.2f} ms ({mk / w_seek:.3f} ms per window)   "
          f"ratio {mk / mf:.2f} at a ratio of windows decoded of {w_seek / w_fixed:.2f} and of groups of {groups_seek / groups_fixed:.2f}", flush=True)
nat.close()
ctx.close()
