#!/usr/bin/env python3
"""The price of the temperature fallback: one rt_stt_transcribe_ex call over 32 one-window clips in which EVERY window falls back
once (a scripted ratio fails each window's first attempt; the second, best_of 5 sampled rows at temperature 0.2, stands), against the
same call with no policy set and against a policy that never triggers.  The workload of tools/bench_stt_beam.py: Whisper-tiny
dimensions on seeded weights, synthetic voiced clips of 4 s at 24 kHz in HBM, max_new_tokens 16, beam 5; five alternating triples in
one process.  The measuring process is a child started under `timeout`, so a hang ends it; this process never opens the GPU.
    python tools/bench_stt_fallback.py [n_clips] [seconds] [max_new_tokens] [--beam N] [--best-of N] [--limit SECONDS]"""
import os, subprocess, sys, time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
argv = sys.argv[1:]


def opt(name, default):
    return int(argv[argv.index(name) + 1]) if name in argv else default


BEAM, BEST_OF, LIMIT = opt("--beam", 5), opt("--best-of", 5), opt("--limit", 300)
ARGS = [a for i, a in enumerate(argv) if not a.startswith("--") and (i == 0 or not argv[i - 1].startswith("--"))]
N = int(ARGS[0]) if len(ARGS) > 0 else 32
SECONDS = float(ARGS[1]) if len(ARGS) > 1 else 4.0
MAX_NEW = int(ARGS[2]) if len(ARGS) > 2 else 16
SR, ROUNDS = 24000, 5

if "--child" not in argv:
    rc = subprocess.run(["timeout", "-k", "10", str(LIMIT), sys.executable, os.path.abspath(__file__), *argv, "--child"]).returncode
    sys.exit(rc)

sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from rho_tts_amd import _native  # noqa: E402
from rho_tts_amd import stt as S  # noqa: E402


def voiced(seconds, f0, seed):
    t = np.arange(int(seconds * SR)) / SR
    x = 0.3 * sum(np.sin(2 * np.pi * f0 * (k + 1) * t) / (k + 1) for k in range(5)) * (0.6 + 0.4 * np.sin(2 * np.pi * 3 * t))
    x[: int(0.1 * SR)] = 0.0
    return (x + 1e-3 * np.random.default_rng(seed).standard_normal(x.shape[0])).astype(np.float32)


if not torch.cuda.is_available():
    sys.exit("bench_stt_fallback.py measures on the GPU; there is none here")
ctx = _native.Context(0)
cfg = S.SttConfig(max_new_tokens=MAX_NEW)
nat = S.NativeSTT(ctx, cfg, S.synthetic_state(cfg, 789, device="cuda"))
clips = [torch.from_numpy(voiced(SECONDS, 110.0 + 7.0 * c, c)).cuda() for c in range(N)]
windows = sum(nat.windows(x.numel(), SR) for x in clips)
torch.cuda.synchronize()
per_group = 32 // max(BEAM, BEST_OF)


class Once:
    """Fails the first attempt of every window: per group of g windows the loop asks for all g, then for the g that failed."""

    def __init__(self):
        self.plan = []
        self.cb = S.RATIO_FN(lambda p_ids, n, user: self.plan.pop(0) if self.plan else 1.0)

    def arm(self):
        self.plan = []
        for at in range(0, windows, per_group):
            g = min(per_group, windows - at)
            self.plan += [9.0] * g + [1.0] * g


once = Once()
call = lambda: nat.transcribe_ids_ex(clips, SR, BEAM, no_speech=False)          # noqa: E731


def no_policy():
    nat.set_fallback(None)
    return call()


def idle_policy():
    nat.set_fallback((0.0, 0.2), BEST_OF, logprob_threshold=None, ratio=S.RATIO_FN(lambda p_ids, n, user: 1.0))
    return call()


def every_window_once():
    once.arm()
    nat.set_fallback((0.0, 0.2), BEST_OF, logprob_threshold=None, ratio=once.cb)
    return call()


what = lambda clips_out: [(c.ids, c.score) for c in clips_out]          # noqa: E731
base = what(no_policy())
if what(idle_policy()) != base:
    sys.exit("a policy that never triggers changed the result")
every_window_once()
rep = nat.fallback_report()
if len(rep) != windows or any(w.attempts != 2 for w in rep):
    sys.exit(f"not every window fell back once: attempts {sorted({w.attempts for w in rep})} over {len(rep)} of {windows} windows")
print(f"{N} clips of {SECONDS:g} s at {SR} Hz, {windows} windows, max_new_tokens {MAX_NEW}, beam {BEAM}, best_of {BEST_OF}: {per_group} windows per group, "
      f"{-(-windows // per_group)} groups; every window: 2 attempts, the second at temperature 0.2", flush=True)
t = {"no policy": [], "policy, never triggers": [], "every window falls back once": []}
for r in range(ROUNDS):
    for name, fn in zip(t, (no_policy, idle_policy, every_window_once)):
        t0 = time.perf_counter()
        fn()
        t[name].append((time.perf_counter() - t0) * 1e3)
    print(f"round {r + 1}: " + "   ".join(f"{k} {v[-1]:8.2f} ms" for k, v in t.items()), flush=True)
med = {k: sorted(v)[ROUNDS // 2] for k, v in t.items()}
print("median: " + "   ".join(f"{k} {v:.2f} ms" for k, v in med.items()) +
      f"   fallback / no policy {med['every window falls back once'] / med['no policy']:.2f}")
nat.close()
ctx.close()
