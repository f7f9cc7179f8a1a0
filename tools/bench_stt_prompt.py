#!/usr/bin/env python3
"""The seek call (NativeSTT.transcribe_ids_seek, width 5 unless given) under a prompt policy against the same call without one, in one
process and alternating: Whisper-tiny dimensions on seeded weights, synthetic voiced clips of 90 s at 24 kHz in HBM.
  plain        no policy: the launches of the parent of this feature
  conditioned  NativeSTT.set_prompt(condition_on_previous=True)
  initial      ... with an initial prompt of the full cap (223 ids): every window decodes behind 227 tokens
  uniform      `initial` with the gather between beam steps in its uniform form (rt_debug_tune 3300): the A/B of the ranged form
The gather of one step on its own, ranged against uniform, by device events (rt_bench_stt_gather).
And the ragged prefix pass on its own (rt_debug_stt_prompt_prefix: front end, encoder and the pass): one group's windows behind 227
tokens each against the same windows behind 3, whose difference is what the prompt rows cost.
    python tools/bench_stt_prompt.py [n_clips] [seconds] [max_new_tokens] [--beam N]"""
import ctypes as C
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from rho_tts_amd import _native
from rho_tts_amd import stt as S

argv = sys.argv[1:]
BEAM = int(argv[argv.index("--beam") + 1]) if "--beam" in argv else 5
ARGS = [a for i, a in enumerate(argv) if not a.startswith("--") and (i == 0 or argv[i - 1] != "--beam")]
N = int(ARGS[0]) if len(ARGS) > 0 else 32 // BEAM
SECONDS = float(ARGS[1]) if len(ARGS) > 1 else 90.0
MAX_NEW = int(ARGS[2]) if len(ARGS) > 2 else 64
SR, ROUNDS = 24000, 5


def voiced(seconds, f0, seed):
    t = np.arange(int(seconds * SR)) / SR
    x = 0.3 * sum(np.sin(2 * np.pi * f0 * (k + 1) * t) / (k + 1) for k in range(5)) * (0.6 + 0.4 * np.sin(2 * np.pi * 3 * t))
    x[: int(0.1 * SR)] = 0.0
    return (x + 1e-3 * np.random.default_rng(seed).standard_normal(x.shape[0])).astype(np.float32)


if not torch.cuda.is_available():
    sys.exit("bench_stt_prompt.py measures on the GPU; there is none here")
ctx = _native.Context(0)
cfg = S.SttConfig(max_new_tokens=MAX_NEW, timestamp_begin=50364)
nat = S.NativeSTT(ctx, cfg, S.synthetic_state(cfg, 789, device="cuda"))
clips = [torch.from_numpy(voiced(SECONDS, 110.0 + 7.0 * c, c)).cuda() for c in range(N)]
cap = cfg.n_text_ctx // 2 - 1
initial = [int(t) for t in np.random.default_rng(20).integers(0, cfg.eos_id, cap)]
torch.cuda.synchronize()
lib = ctx.lib


def run(mode):
    ranged = (1, 0)[mode == "uniform"]
    lib.rt_debug_tune(3300 + ranged, 0)
    if mode == "plain":
        nat.set_prompt(None)
    else:
        nat.set_prompt(None if mode == "conditioned" else initial, condition_on_previous=True)
    t0 = time.perf_counter()
    out = nat.transcribe_ids_seek(clips, SR, BEAM, no_speech=False)
    return (time.perf_counter() - t0) * 1e3, out


MODES = ("plain", "conditioned", "initial", "uniform")
first = {m: run(m)[1] for m in MODES}                      # (warm: every buffer set is grown here, not in a timed call)
free = torch.cuda.mem_get_info()[0]
steps = {m: sum(max(c.windows[k].n_ids for c in first[m] if k < len(c.windows)) for k in range(max(len(c.windows) for c in first[m]))) for m in MODES}
for m in MODES:
    wins = [w for c in first[m] for w in c.windows]
    print(f"{m:12s}: {len(wins)} windows in {max(len(c.windows) for c in first[m])} rounds, prompts {min(w.prompt_len for w in wins)} .. {max(w.prompt_len for w in wins)} ids, "
          f"{sum(w.n_ids for w in wins)} ids decoded, {steps[m]} steps", flush=True)

def shown(clips_):
    """A call's result without the windows' no-speech probabilities (NaN here, which never compares equal)."""
    return [(c.ids, c.score, [(g.start_tick, g.end_tick, g.ids) for g in c.segments], [(w.offset, w.n_ids, w.logprob, w.advance, w.prompt_len) for w in c.windows])
            for c in clips_]


if shown(first["uniform"]) != shown(first["initial"]):
    sys.exit("the uniform gather gives other results than the ranged one")
print(f"{N} clips of {SECONDS:g} s at {SR} Hz, beam {BEAM}, max_new_tokens {MAX_NEW}; device memory free after the warm-up {free / 2**30:.2f} GiB", flush=True)
times = {m: [] for m in MODES}
for r in range(ROUNDS):
    for m in MODES:
        times[m].append(run(m)[0])
    print(f"round {r + 1}: " + "   ".join(f"{m} {times[m][-1]:8.2f} ms" for m in MODES), flush=True)
med = {m: sorted(times[m])[ROUNDS // 2] for m in MODES}
print("median: " + "   ".join(f"{m} {med[m]:.2f} ms (spread {max(times[m]) - min(times[m]):.2f})" for m in MODES))
print(f"conditioned / plain {med['conditioned'] / med['plain']:.3f}   initial / plain {med['initial'] / med['plain']:.3f}")
print(f"whole call, uniform - ranged gather: {med['uniform'] - med['initial']:.2f} ms over {steps['initial']} steps")
lib.rt_debug_tune(3301, 0)
nat.set_prompt(None)

# the gather of one step on its own (device events, 200 launches back to back): the rows of one group behind the longest prefix
lib.rt_bench_stt_gather.argtypes = [C.c_void_p] + [C.c_int32] * 8 + [C.POINTER(C.c_double)] * 2
rows, longest = (32 // BEAM) * BEAM, cfg.n_text_ctx // 2 + len(cfg.prefix) - 1
for step in (1, 8, 32, MAX_NEW - 1, cfg.n_text_ctx - longest - 1):
    ur, uu = C.c_double(), C.c_double()
    ctx.check(lib.rt_bench_stt_gather(ctx.handle, cfg.dec_layers, rows, cfg.heads, cfg.n_text_ctx, cfg.d_model // cfg.heads, longest, step, 200, C.byref(ur), C.byref(uu)),
              "rt_bench_stt_gather")
    print(f"gather of {rows} rows behind a prefix of {longest}, step {step:3d}: ranged {ur.value:7.2f} us   uniform {uu.value:7.2f} us per launch", flush=True)

# the ragged prefix pass of one group on its own
i32, vp = C.c_int32, C.c_void_p
lib.rt_debug_stt_prompt_prefix.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_int64), i32, i32, C.POINTER(i32), C.POINTER(i32), vp]
forced = [int(t) for t in cfg.prefix[:-1]]
xs, n, ptrs, lens = nat._clips(clips)
logits = torch.empty(n, cfg.vocab, dtype=torch.float32, device="cuda")


def prefix_pass(row):
    flat = row * n
    t0 = time.perf_counter()
    ctx.check(lib.rt_debug_stt_prompt_prefix(nat.handle, ptrs, lens, n, SR, (i32 * len(flat))(*flat), (i32 * n)(*[len(row)] * n), vp(logits.data_ptr())), "rt_debug_stt_prompt_prefix")
    return (time.perf_counter() - t0) * 1e3


long_row, short_row = [cfg.sot_prev_id] + initial + forced, forced
prefix_pass(long_row), prefix_pass(short_row)
t_long, t_short = [], []
for r in range(ROUNDS):
    t_long.append(prefix_pass(long_row))
    t_short.append(prefix_pass(short_row))
ml, ms = sorted(t_long)[ROUNDS // 2], sorted(t_short)[ROUNDS // 2]
print(f"front end + encoder + prefix pass of {n} windows: {len(long_row)} tokens each {ml:.2f} ms (spread {max(t_long) - min(t_long):.2f}), {len(short_row)} tokens each {ms:.2f} ms "
      f"(spread {max(t_short) - min(t_short):.2f}): the prompt rows cost {ml - ms:.2f} ms per group of {n} windows ({n * len(long_row)} rows)")
nat.close()
ctx.close()
