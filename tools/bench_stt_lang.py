#!/usr/bin/env python3
"""What language detection costs a validation chunk: the existing beam call (NativeSTT.transcribe_ids_beam) against
rt_stt_transcribe_ex with the language given - with and without the windows' no-speech probabilities - and with every clip's
language detected, interleaved in one process.  The workload of tools/bench_stt_beam.py: Whisper-tiny dimensions on seeded weights,
32 synthetic voiced clips of 4 s at 24 kHz in HBM, max_new_tokens 16, width 5.  Before anything is timed: the language given as the
configuration's own returns the ids and scores of the beam call, and detection returns those of its detected ids given.
    python tools/bench_stt_lang.py [n_clips] [seconds] [max_new_tokens] [--beam N]"""
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
SR, ROUNDS = 24000, 7


def voiced(seconds, f0, seed):
    t = np.arange(int(seconds * SR)) / SR
    x = 0.3 * sum(np.sin(2 * np.pi * f0 * (k + 1) * t) / (k + 1) for k in range(5)) * (0.6 + 0.4 * np.sin(2 * np.pi * 3 * t))
    x[: int(0.1 * SR)] = 0.0
    return (x + 1e-3 * np.random.default_rng(seed).standard_normal(x.shape[0])).astype(np.float32)


if not torch.cuda.is_available():
    sys.exit("bench_stt_lang.py measures on the GPU; there is none here")
ctx = _native.Context(0)
cfg = S.SttConfig(max_new_tokens=MAX_NEW)
nat = S.NativeSTT(ctx, cfg, S.synthetic_state(cfg, 789, device="cuda"))
clips = [torch.from_numpy(voiced(SECONDS, 110.0 + 7.0 * c, c)).cuda() for c in range(N)]
windows = sum(nat.windows(x.numel(), SR) for x in clips)
torch.cuda.synchronize()
calls = [
    ("beam (existing entry)", lambda: nat.transcribe_ids_beam(clips, SR, BEAM)),
    ("ex, language given", lambda: nat.transcribe_ids_ex(clips, SR, BEAM, "en", no_speech=False)),
    ("ex, given + no-speech", lambda: nat.transcribe_ids_ex(clips, SR, BEAM, "en", no_speech=True)),
    ("ex, language detected", lambda: nat.transcribe_ids_ex(clips, SR, BEAM, "auto", no_speech=True)),
    ("detect_language alone", lambda: nat.detect_language(clips, SR)),
]
ids, scores = calls[0][1]()
given = calls[1][1]()
if [c.ids for c in given] != ids or [c.score for c in given] != scores:
    sys.exit("the language given as the configuration's own differs from the beam call")
auto = calls[3][1]()
again = nat.transcribe_ids_ex(clips, SR, BEAM, [c.language for c in auto])
if [(c.ids, c.score) for c in auto] != [(c.ids, c.score) for c in again]:
    sys.exit("detection differs from its detected ids given")
langs = sorted({cfg.language_code(c.language) for c in auto})
per_group = 32 // BEAM
print(f"{N} clips of {SECONDS:g} s at {SR} Hz, {windows} windows, max_new_tokens {MAX_NEW}, beam {BEAM}: {per_group} windows per group, "
      f"{-(-windows // per_group)} groups; 99 languages, detected {langs}; language probability {min(c.language_prob for c in auto):.3f} .. "
      f"{max(c.language_prob for c in auto):.3f}; no-speech {min(w.no_speech_prob for c in auto for w in c.windows):.2e} .. "
      f"{max(w.no_speech_prob for c in auto for w in c.windows):.2e}", flush=True)
times = [[] for _ in calls]
for r in range(ROUNDS):
    row = []
    for k, (_, f) in enumerate(calls):
        t0 = time.perf_counter()
        f()
        times[k].append((time.perf_counter() - t0) * 1e3)
        row.append(f"{times[k][-1]:8.2f}")
    print(f"round {r + 1}: " + "  ".join(row) + " ms", flush=True)
med = [sorted(t)[ROUNDS // 2] for t in times]
for (name, _), t, m in zip(calls, times, med):
    print(f"{name:24s} median {m:8.2f} ms  min {min(t):8.2f}  max {max(t):8.2f}  vs the beam call {m / med[0]:6.3f}x ({m - med[0]:+7.2f} ms)")
nat.close()
ctx.close()
