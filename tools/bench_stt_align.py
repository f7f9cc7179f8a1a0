#!/usr/bin/env python3
"""Word times against the transcription they follow: NativeSTT.align_ids (rt_stt_align: one encoder pass, one teacher-forced decoder
pass with the capture launches, normalisation, filter and the paths) against NativeSTT.transcribe_ids_batch (rt_stt_transcribe_batch:
one encoder pass and a decoder step per generated token) on the same windows.  Whisper-tiny dimensions on seeded weights, 32 windows
of 30 s at 24 kHz in HBM, 60 text ids each (the batch call decodes 60 tokens per window: max_new_tokens 60); five alternating pairs
in one process.  Within the alignment call, events around the launches it adds (rt_debug_stt_align_timing): the capture launches,
statistics + matrix, the paths.
    python tools/bench_stt_align.py [n_windows] [seconds] [n_ids]"""
import ctypes as C
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from rho_tts_amd import _native
from rho_tts_amd import stt as S

ARGS = [a for a in sys.argv[1:] if not a.startswith("--")]
N = int(ARGS[0]) if len(ARGS) > 0 else 32
SECONDS = float(ARGS[1]) if len(ARGS) > 1 else 30.0
N_IDS = int(ARGS[2]) if len(ARGS) > 2 else 60
SR, PAIRS = 24000, 5


def voiced(seconds, f0, seed):
    t = np.arange(int(seconds * SR)) / SR
    x = 0.3 * sum(np.sin(2 * np.pi * f0 * (k + 1) * t) / (k + 1) for k in range(5)) * (0.6 + 0.4 * np.sin(2 * np.pi * 3 * t))
    return (x + 1e-3 * np.random.default_rng(seed).standard_normal(x.shape[0])).astype(np.float32)


if not torch.cuda.is_available():
    sys.exit("bench_stt_align.py measures on the GPU; there is none here")
ctx = _native.Context(0)
cfg = S.SttConfig(max_new_tokens=N_IDS)
nat = S.NativeSTT(ctx, cfg, S.synthetic_state(cfg, 789, device="cuda"))
lib = ctx.lib
lib.rt_debug_stt_align_timing.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]
clips = [torch.from_numpy(voiced(SECONDS, 110.0 + 7.0 * c, c)).cuda() for c in range(N)]
g = np.random.default_rng(1)
ids = [[int(t) for t in g.integers(0, cfg.eos_id, N_IDS)] for _ in range(N)]
torch.cuda.synchronize()
align = lambda: nat.align_ids(clips, SR, ids)                       # noqa: E731
decode = lambda: nat.transcribe_ids_batch(clips, SR)                # noqa: E731
free0 = torch.cuda.mem_get_info()[0]
decoded = decode()
free1 = torch.cuda.mem_get_info()[0]
times = align()
free2 = torch.cuda.mem_get_info()[0]
print(f"{N} windows of {SECONDS:g} s at {SR} Hz, {N_IDS} text ids each, {len(cfg.aligned_heads)} alignment heads, median width {cfg.median_filter_width}; "
      f"the decode call emitted {min(map(len, decoded))} .. {max(map(len, decoded))} ids per window; frames per window {times[0].n_frames}", flush=True)
print(f"device memory: the decode call took {(free0 - free1) / 2**20:.0f} MiB, the first alignment call {(free1 - free2) / 2**20:.0f} MiB more", flush=True)
t_al, t_de = [], []
for p in range(PAIRS):
    t0 = time.perf_counter()
    decode()
    t1 = time.perf_counter()
    align()
    t2 = time.perf_counter()
    t_de.append((t1 - t0) * 1e3)
    t_al.append((t2 - t1) * 1e3)
    print(f"pair {p + 1}: decode {t_de[-1]:9.2f} ms   align {t_al[-1]:8.2f} ms   align / decode {t_al[-1] / t_de[-1]:5.2f}   align faster: {t_al[-1] < t_de[-1]}", flush=True)
md, ma = sorted(t_de)[PAIRS // 2], sorted(t_al)[PAIRS // 2]
print(f"median: decode {md:.2f} ms   align {ma:.2f} ms ({ma / N:.3f} ms per window)   align / decode {ma / md:.2f}")
print(f"align faster in every pair: {all(a < d for a, d in zip(t_al, t_de))}")
cap, mat, dtw = C.c_double(), C.c_double(), C.c_double()
ctx.check(lib.rt_debug_stt_align_timing(nat.handle, 1, None, None, None), "rt_debug_stt_align_timing")
REPS = 3
for _ in range(REPS):
    align()
ctx.check(lib.rt_debug_stt_align_timing(nat.handle, 0, C.byref(cap), C.byref(mat), C.byref(dtw)), "rt_debug_stt_align_timing")
print(f"within one alignment call (events, mean of {REPS}): capture launches {cap.value / REPS:.3f} ms   statistics + matrix {mat.value / REPS:.3f} ms   "
      f"paths {dtw.value / REPS:.3f} ms")
nat.close()
ctx.close()
