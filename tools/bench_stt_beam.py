#!/usr/bin/env python3
"""Transcription of one validation chunk by beam search (NativeSTT.transcribe_ids_beam, width 5 unless given) against the greedy
batched call (NativeSTT.transcribe_ids_batch) of the same build.  The workload of tools/bench_stt.py: Whisper-tiny dimensions on
seeded weights, 32 synthetic voiced clips of 4 s at 24 kHz in HBM, max_new_tokens 16; five alternating pairs in one process.  Width 1
through the beam call must give the greedy ids: checked before anything is timed.
    python tools/bench_stt_beam.py [n_clips] [seconds] [max_new_tokens] [--beam N]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from rho_tts_amd import _native
from rho_tts_amd import stt as S

argv = sys.argv[1:]
BEAM = int(argv[argv.index("--beam") + 1]) if "--beam" in argv else 5
ARGS = [a for i, a in enumerate(argv) if not a.startswith("--") and (i == 0 or argv[i - 1] != "--beam")]
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
    sys.exit("bench_stt_beam.py measures on the GPU; there is none here")
ctx = _native.Context(0)
cfg = S.SttConfig(max_new_tokens=MAX_NEW)
nat = S.NativeSTT(ctx, cfg, S.synthetic_state(cfg, 789, device="cuda"))
clips = [torch.from_numpy(voiced(SECONDS, 110.0 + 7.0 * c, c)).cuda() for c in range(N)]
windows = sum(nat.windows(x.numel(), SR) for x in clips)
torch.cuda.synchronize()
greedy = lambda: nat.transcribe_ids_batch(clips, SR)               # noqa: E731
beam = lambda: nat.transcribe_ids_beam(clips, SR, BEAM)            # noqa: E731
g = greedy()
free0 = torch.cuda.mem_get_info()[0]
if nat.transcribe_ids_beam(clips, SR, 1)[0] != g:                  # (the first beam call: 32 windows x 1 beam = a full group of 32 rows)
    sys.exit("width 1 through the beam call differs from the greedy batched call")
free1 = torch.cuda.mem_get_info()[0]
ids, scores = beam()
per_group = 32 // BEAM
print(f"{N} clips of {SECONDS:g} s at {SR} Hz, {windows} windows, max_new_tokens {MAX_NEW}, beam {BEAM}: {per_group} windows = {per_group * BEAM} rows per "
      f"group, {-(-windows // per_group)} groups; {sum(1 for a, b in zip(ids, g) if a != b)} of {N} clips differ from greedy; ids per clip "
      f"{min(map(len, ids))} .. {max(map(len, ids))} (greedy {min(map(len, g))} .. {max(map(len, g))}); score {min(scores):.3f} .. {max(scores):.3f}", flush=True)
print(f"device memory taken by the first beam call (32 rows) beyond the greedy group's: {(free0 - free1) / 2**20:.0f} MiB = "
      f"{(free0 - free1) / 32 / 1e6:.1f} MB per row", flush=True)
t_g, t_b = [], []
for p in range(PAIRS):
    t0 = time.perf_counter()
    greedy()
    t1 = time.perf_counter()
    beam()
    t2 = time.perf_counter()
    t_g.append((t1 - t0) * 1e3)
    t_b.append((t2 - t1) * 1e3)
    print(f"pair {p + 1}: greedy batch {t_g[-1]:8.2f} ms   beam {BEAM} {t_b[-1]:8.2f} ms   ratio {t_b[-1] / t_g[-1]:5.2f}", flush=True)
mg, mb = sorted(t_g)[PAIRS // 2], sorted(t_b)[PAIRS // 2]
print(f"median: greedy batch {mg:.2f} ms ({mg / N:.3f} ms per clip)   beam {BEAM} {mb:.2f} ms ({mb / N:.3f} ms per clip)   ratio {mb / mg:.2f}")
nat.close()
ctx.close()
