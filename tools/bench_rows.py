#!/usr/bin/env python3
"""Decode-frame time against the number of decode rows (1.7B shapes, synthetic weights, the bench's 30-s voice): one static batch
of R ten-word texts for F and for 2F frames; (t(2F) - t(F)) / F is the time of a frame without the prompt prefill.  Alternating
passes over the widths, median with min and max; the last column is what engine.FRAME_COST holds (relative to 32 rows)."""
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

WIDTHS = (32, 64, 96, 128)
F = 40
cfg = config.PRESETS[sys.argv[1] if len(sys.argv) > 1 else "1.7b"]()
eng = Engine(cfg=cfg, model_path=cfg.name, device_ordinal=0, max_batch=128, synthetic=True)
for code in [c for c in (sys.argv[2] if len(sys.argv) > 2 else "").split(",") if c]:
    eng.ctx.lib.rt_debug_tune(int(code), 0)
eng.set_voice_from_audio(synthetic_reference_clip(30.0, cfg.sample_rate, 789), " ".join(WORDS[i % len(WORDS)] for i in range(75)))
ids = [eng.tokenizer.encode(t) for t in sentences(128, 10, seed=789)]


def run(rows, frames):
    torch.cuda.synchronize()
    eng.ctx.synchronize()
    t0 = time.perf_counter()
    eng.model.generate(ids[:rows], [frames] * rows, eng.params.talker(), eng.params.predictor(), seed=789, item_ids=list(range(rows)), ignore_eos=True)
    eng.ctx.synchronize()
    return (time.perf_counter() - t0) * 1e3


per = {r: [] for r in WIDTHS}
for rep in range(6):
    for r in WIDTHS:
        a, b = run(r, F), run(r, 2 * F)
        if rep:                                 # (the first pass captures the graphs)
            per[r].append((b - a) / F)
base = statistics.median(per[32])
for r in WIDTHS:
    m = statistics.median(per[r])
    print(f"rows {r:3d}: frame {m:7.3f} ms (min {min(per[r]):.3f} max {max(per[r]):.3f})   per row-frame {m / r * 1e3:7.2f} us   relative to 32 rows {m / base:.3f}",
          flush=True)
eng.close()
