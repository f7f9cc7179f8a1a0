#!/usr/bin/env python3
"""What mixing voices costs a decode frame (1.7B shapes, synthetic weights): one static batch of 32 ten-word texts on 32 rows,
44 frames, with 1, 2, 4 and 8 voices spread evenly over the rows in 4-row blocks - every voice a 30-s clone (a prefix of about 460
rows).  As tools/bench_rows.py: each width runs F and 2F frames and (t(2F) - t(F)) / F is the frame without the prompt prefill;
alternating passes, median with min and max.  "1 voice" is this build's single-voice run (no item voices: the launches a run took
before there was a bank); "1 voice, named" hands the same voice to every item (the same launches by construction).
Then the talker's attention launch on its own, back to back (rt_bench_attention_fused_voices): the single-voice kernel against the
multi-voice kernel at 32 rows, a 460-row prefix per voice, 44 own positions, 28 cache regions, for 1, 2, 4 and 8 voices.

    python tools/bench_voices.py [preset] [tune codes, comma separated - e.g. 1501 for the matrix-core decode attention]"""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from bench import WORDS, sentences  # noqa: E402
from rho_tts_amd import config  # noqa: E402
from rho_tts_amd.engine import Engine  # noqa: E402
from rho_tts_amd.voice import synthetic_reference_clip  # noqa: E402

ROWS, F, VOICES = 32, 44, (1, 2, 4, 8)
cfg = config.PRESETS[sys.argv[1] if len(sys.argv) > 1 else "1.7b"]()
eng = Engine(cfg=cfg, model_path=cfg.name, device_ordinal=0, max_batch=ROWS, synthetic=True, max_voices=max(VOICES))
for code in [c for c in (sys.argv[2] if len(sys.argv) > 2 else "").split(",") if c]:
    eng.ctx.lib.rt_debug_tune(int(code), 0)
ref_text = " ".join(WORDS[i % len(WORDS)] for i in range(75))
lens = [eng.set_voice_from_audio(synthetic_reference_clip(30.0, cfg.sample_rate, 789), ref_text)]
for v in range(1, max(VOICES)):
    eng.add_voice(f"v{v}", eng.conditioning_from_audio(synthetic_reference_clip(30.0, cfg.sample_rate, 789 + v), ref_text))
    lens.append(eng._prefix_len[v])
print(f"prefix rows per voice: {lens}", flush=True)
ids = [eng.tokenizer.encode(t) for t in sentences(ROWS, 10, seed=789)]


def run(voices, frames):
    torch.cuda.synchronize()
    eng.ctx.synchronize()
    t0 = time.perf_counter()
    eng.model.generate(ids, [frames] * ROWS, eng.params.talker(), eng.params.predictor(), seed=789, item_ids=list(range(ROWS)), ignore_eos=True, voices=voices)
    eng.ctx.synchronize()
    return (time.perf_counter() - t0) * 1e3


cases = [("1 voice", None), ("1 voice, named", [0] * ROWS)] + [(f"{n} voices", [(r // 4) % n for r in range(ROWS)]) for n in VOICES[1:]]
per = {name: [] for name, _ in cases}
for rep in range(6):
    for name, voices in cases:
        a, b = run(voices, F), run(voices, 2 * F)
        if rep:                                 # (the first pass captures the graphs)
            per[name].append((b - a) / F)
base = statistics.median(per["1 voice"])
for name, _ in cases:
    m = statistics.median(per[name])
    print(f"{name:15s}: frame {m:7.3f} ms (min {min(per[name]):.3f} max {max(per[name]):.3f})   relative to the single-voice run {m / base:.4f}", flush=True)
eng.close()

import ctypes as C  # noqa: E402

from rho_tts_amd import _native  # noqa: E402

ctx = _native.Context(0)
for code in [c for c in (sys.argv[2] if len(sys.argv) > 2 else "").split(",") if c]:
    ctx.lib.rt_debug_tune(int(code), 0)
ctx.lib.rt_bench_attention_fused_voices.argtypes = [C.c_void_p] + [C.c_int32] * 9 + [C.POINTER(C.c_double)] * 2
t = cfg.talker
for n in VOICES:
    one, many = C.c_double(), C.c_double()
    ctx.check(ctx.lib.rt_bench_attention_fused_voices(ctx.handle, ROWS, t.heads, t.kv_heads, t.head_dim, 460, F, n, t.layers, 2000, C.byref(one), C.byref(many)),
              "rt_bench_attention_fused_voices")
    print(f"attention launch, {n} voice(s): single-voice kernel {one.value:6.2f} us, multi-voice kernel {many.value:6.2f} us  ({many.value / one.value:.3f})", flush=True)
ctx.close()
